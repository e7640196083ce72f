// Instantiations of bf_nd (bf_nd.h), forward and gradient, for m = 9..12.
#include "bf_nd.h"

namespace nngp {

bool bf_nd_launch_b(const NdArgs& a, bool grad, hipStream_t s) {
    return launch_nd_if<9>(a, grad, s) ||
           launch_nd_if<10>(a, grad, s) ||
           launch_nd_if<11>(a, grad, s) ||
           launch_nd_if<12>(a, grad, s);
}

}  // namespace nngp
