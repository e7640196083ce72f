// Instantiations of bf_grad_matern (bf_grad_matern.h) for m = 21..24.
#include "bf_grad_matern.h"

namespace nngp {

bool bf_grad_matern_launch_e(const GradMaternArgs& a, hipStream_t s) {
    return launch_grad_matern_if<21>(a, s) ||
           launch_grad_matern_if<22>(a, s) ||
           launch_grad_matern_if<23>(a, s) ||
           launch_grad_matern_if<24>(a, s);
}

}  // namespace nngp
