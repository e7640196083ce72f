// Instantiations of bf_dphi (bf_dphi.h) for m = 25..27.
#include "bf_dphi.h"

namespace nngp {

bool bf_dphi_launch_f(const DphiArgs& a, hipStream_t s) {
    return launch_dphi_if<25>(a, s) ||
           launch_dphi_if<26>(a, s) ||
           launch_dphi_if<27>(a, s);
}

}  // namespace nngp
