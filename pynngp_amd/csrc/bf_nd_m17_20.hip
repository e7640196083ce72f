// Instantiations of bf_nd (bf_nd.h), forward and gradient, for m = 17..20.
#include "bf_nd.h"

namespace nngp {

bool bf_nd_launch_d(const NdArgs& a, bool grad, hipStream_t s) {
    return launch_nd_if<17>(a, grad, s) ||
           launch_nd_if<18>(a, grad, s) ||
           launch_nd_if<19>(a, grad, s) ||
           launch_nd_if<20>(a, grad, s);
}

}  // namespace nngp
