// Instantiations of bf_dphi (bf_dphi.h) for m = 28..30.
#include "bf_dphi.h"

namespace nngp {

bool bf_dphi_launch_g(const DphiArgs& a, hipStream_t s) {
    return launch_dphi_if<28>(a, s) ||
           launch_dphi_if<29>(a, s) ||
           launch_dphi_if<30>(a, s);
}

}  // namespace nngp
