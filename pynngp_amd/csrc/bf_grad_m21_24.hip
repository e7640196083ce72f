// Instantiations of bf_grad (bf_grad.h) for m = 21..24.
#include "bf_grad.h"

namespace nngp {

bool bf_grad_launch_e(const GradArgs& a, hipStream_t s) {
    return launch_grad_if<21>(a, s) ||
           launch_grad_if<22>(a, s) ||
           launch_grad_if<23>(a, s) ||
           launch_grad_if<24>(a, s);
}

}  // namespace nngp
