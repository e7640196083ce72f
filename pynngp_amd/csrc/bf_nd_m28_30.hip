// Instantiations of bf_nd (bf_nd.h), forward and gradient, for m = 28..30.
#include "bf_nd.h"

namespace nngp {

bool bf_nd_launch_g(const NdArgs& a, bool grad, hipStream_t s) {
    return launch_nd_if<28>(a, grad, s) ||
           launch_nd_if<29>(a, grad, s) ||
           launch_nd_if<30>(a, grad, s);
}

}  // namespace nngp
