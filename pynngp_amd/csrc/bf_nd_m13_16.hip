// Instantiations of bf_nd (bf_nd.h), forward and gradient, for m = 13..16.
#include "bf_nd.h"

namespace nngp {

bool bf_nd_launch_c(const NdArgs& a, bool grad, hipStream_t s) {
    return launch_nd_if<13>(a, grad, s) ||
           launch_nd_if<14>(a, grad, s) ||
           launch_nd_if<15>(a, grad, s) ||
           launch_nd_if<16>(a, grad, s);
}

}  // namespace nngp
