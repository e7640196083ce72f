// Instantiations of bf_dphi (bf_dphi.h) for m = 21..24.
#include "bf_dphi.h"

namespace nngp {

bool bf_dphi_launch_e(const DphiArgs& a, hipStream_t s) {
    return launch_dphi_if<21>(a, s) ||
           launch_dphi_if<22>(a, s) ||
           launch_dphi_if<23>(a, s) ||
           launch_dphi_if<24>(a, s);
}

}  // namespace nngp
