// Instantiations of bf_nd (bf_nd.h), forward and gradient, for m = 1..8.
#include "bf_nd.h"

namespace nngp {

bool bf_nd_launch_a(const NdArgs& a, bool grad, hipStream_t s) {
    return launch_nd_if<1>(a, grad, s) ||
           launch_nd_if<2>(a, grad, s) ||
           launch_nd_if<3>(a, grad, s) ||
           launch_nd_if<4>(a, grad, s) ||
           launch_nd_if<5>(a, grad, s) ||
           launch_nd_if<6>(a, grad, s) ||
           launch_nd_if<7>(a, grad, s) ||
           launch_nd_if<8>(a, grad, s);
}

}  // namespace nngp
