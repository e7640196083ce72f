// Instantiations of bf_nd (bf_nd.h), forward and gradient, for m = 21..24.
#include "bf_nd.h"

namespace nngp {

bool bf_nd_launch_e(const NdArgs& a, bool grad, hipStream_t s) {
    return launch_nd_if<21>(a, grad, s) ||
           launch_nd_if<22>(a, grad, s) ||
           launch_nd_if<23>(a, grad, s) ||
           launch_nd_if<24>(a, grad, s);
}

}  // namespace nngp
