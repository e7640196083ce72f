// Instantiations of bf_nd (bf_nd.h), forward and gradient, for m = 31..32.
#include "bf_nd.h"

namespace nngp {

bool bf_nd_launch_h(const NdArgs& a, bool grad, hipStream_t s) {
    return launch_nd_if<31>(a, grad, s) ||
           launch_nd_if<32>(a, grad, s);
}

}  // namespace nngp
