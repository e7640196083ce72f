// Instantiations of bf_dphi (bf_dphi.h) for m = 1..8.
#include "bf_dphi.h"

namespace nngp {

bool bf_dphi_launch_a(const DphiArgs& a, hipStream_t s) {
    return launch_dphi_if<1>(a, s) ||
           launch_dphi_if<2>(a, s) ||
           launch_dphi_if<3>(a, s) ||
           launch_dphi_if<4>(a, s) ||
           launch_dphi_if<5>(a, s) ||
           launch_dphi_if<6>(a, s) ||
           launch_dphi_if<7>(a, s) ||
           launch_dphi_if<8>(a, s);
}

}  // namespace nngp
