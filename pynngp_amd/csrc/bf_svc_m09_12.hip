// Instantiations of bf_svc (bf_svc.h), forward and gradient, for m = 9..12.
#include "bf_svc.h"

namespace nngp {

bool bf_svc_launch_b(const SvcArgs& a, bool grad, hipStream_t s) {
    return launch_svc_if<9>(a, grad, s) ||
           launch_svc_if<10>(a, grad, s) ||
           launch_svc_if<11>(a, grad, s) ||
           launch_svc_if<12>(a, grad, s);
}

}  // namespace nngp
