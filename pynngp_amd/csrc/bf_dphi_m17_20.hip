// Instantiations of bf_dphi (bf_dphi.h) for m = 17..20.
#include "bf_dphi.h"

namespace nngp {

bool bf_dphi_launch_d(const DphiArgs& a, hipStream_t s) {
    return launch_dphi_if<17>(a, s) ||
           launch_dphi_if<18>(a, s) ||
           launch_dphi_if<19>(a, s) ||
           launch_dphi_if<20>(a, s);
}

}  // namespace nngp
