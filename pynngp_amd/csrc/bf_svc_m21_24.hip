// Instantiations of bf_svc (bf_svc.h), forward and gradient, for m = 21..24.
#include "bf_svc.h"

namespace nngp {

bool bf_svc_launch_e(const SvcArgs& a, bool grad, hipStream_t s) {
    return launch_svc_if<21>(a, grad, s) ||
           launch_svc_if<22>(a, grad, s) ||
           launch_svc_if<23>(a, grad, s) ||
           launch_svc_if<24>(a, grad, s);
}

}  // namespace nngp
