// Instantiations of bf_svc (bf_svc.h), forward and gradient, for m = 28..30.
#include "bf_svc.h"

namespace nngp {

bool bf_svc_launch_g(const SvcArgs& a, bool grad, hipStream_t s) {
    return launch_svc_if<28>(a, grad, s) ||
           launch_svc_if<29>(a, grad, s) ||
           launch_svc_if<30>(a, grad, s);
}

}  // namespace nngp
