// Instantiations of bf_svc (bf_svc.h), forward and gradient, for m = 17..20.
#include "bf_svc.h"

namespace nngp {

bool bf_svc_launch_d(const SvcArgs& a, bool grad, hipStream_t s) {
    return launch_svc_if<17>(a, grad, s) ||
           launch_svc_if<18>(a, grad, s) ||
           launch_svc_if<19>(a, grad, s) ||
           launch_svc_if<20>(a, grad, s);
}

}  // namespace nngp
