// Instantiations of bf_dphi (bf_dphi.h) for m = 31..32.
#include "bf_dphi.h"

namespace nngp {

bool bf_dphi_launch_h(const DphiArgs& a, hipStream_t s) {
    return launch_dphi_if<31>(a, s) ||
           launch_dphi_if<32>(a, s);
}

}  // namespace nngp
