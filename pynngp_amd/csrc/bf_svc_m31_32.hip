// Instantiations of bf_svc (bf_svc.h), forward and gradient, for m = 31..32.
#include "bf_svc.h"

namespace nngp {

bool bf_svc_launch_h(const SvcArgs& a, bool grad, hipStream_t s) {
    return launch_svc_if<31>(a, grad, s) ||
           launch_svc_if<32>(a, grad, s);
}

}  // namespace nngp
