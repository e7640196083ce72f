// Instantiations of bf_svc (bf_svc.h), forward and gradient, for m = 13..16.
#include "bf_svc.h"

namespace nngp {

bool bf_svc_launch_c(const SvcArgs& a, bool grad, hipStream_t s) {
    return launch_svc_if<13>(a, grad, s) ||
           launch_svc_if<14>(a, grad, s) ||
           launch_svc_if<15>(a, grad, s) ||
           launch_svc_if<16>(a, grad, s);
}

}  // namespace nngp
