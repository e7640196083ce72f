// Instantiations of bf_svc (bf_svc.h), forward and gradient, for m = 25..27.
#include "bf_svc.h"

namespace nngp {

bool bf_svc_launch_f(const SvcArgs& a, bool grad, hipStream_t s) {
    return launch_svc_if<25>(a, grad, s) ||
           launch_svc_if<26>(a, grad, s) ||
           launch_svc_if<27>(a, grad, s);
}

}  // namespace nngp
