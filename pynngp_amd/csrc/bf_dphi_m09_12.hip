// Instantiations of bf_dphi (bf_dphi.h) for m = 9..12.
#include "bf_dphi.h"

namespace nngp {

bool bf_dphi_launch_b(const DphiArgs& a, hipStream_t s) {
    return launch_dphi_if<9>(a, s) ||
           launch_dphi_if<10>(a, s) ||
           launch_dphi_if<11>(a, s) ||
           launch_dphi_if<12>(a, s);
}

}  // namespace nngp
