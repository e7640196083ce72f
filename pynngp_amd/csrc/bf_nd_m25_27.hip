// Instantiations of bf_nd (bf_nd.h), forward and gradient, for m = 25..27.
#include "bf_nd.h"

namespace nngp {

bool bf_nd_launch_f(const NdArgs& a, bool grad, hipStream_t s) {
    return launch_nd_if<25>(a, grad, s) ||
           launch_nd_if<26>(a, grad, s) ||
           launch_nd_if<27>(a, grad, s);
}

}  // namespace nngp
