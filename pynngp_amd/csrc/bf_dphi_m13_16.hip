// Instantiations of bf_dphi (bf_dphi.h) for m = 13..16.
#include "bf_dphi.h"

namespace nngp {

bool bf_dphi_launch_c(const DphiArgs& a, hipStream_t s) {
    return launch_dphi_if<13>(a, s) ||
           launch_dphi_if<14>(a, s) ||
           launch_dphi_if<15>(a, s) ||
           launch_dphi_if<16>(a, s);
}

}  // namespace nngp
