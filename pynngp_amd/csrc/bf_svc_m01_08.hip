// Instantiations of bf_svc (bf_svc.h), forward and gradient, for m = 1..8.
#include "bf_svc.h"

namespace nngp {

bool bf_svc_launch_a(const SvcArgs& a, bool grad, hipStream_t s) {
    return launch_svc_if<1>(a, grad, s) ||
           launch_svc_if<2>(a, grad, s) ||
           launch_svc_if<3>(a, grad, s) ||
           launch_svc_if<4>(a, grad, s) ||
           launch_svc_if<5>(a, grad, s) ||
           launch_svc_if<6>(a, grad, s) ||
           launch_svc_if<7>(a, grad, s) ||
           launch_svc_if<8>(a, grad, s);
}

}  // namespace nngp
