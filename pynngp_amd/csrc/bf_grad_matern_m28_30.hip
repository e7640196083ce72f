// Instantiations of bf_grad_matern (bf_grad_matern.h) for m = 28..30.
#include "bf_grad_matern.h"

namespace nngp {

bool bf_grad_matern_launch_g(const GradMaternArgs& a, hipStream_t s) {
    return launch_grad_matern_if<28>(a, s) ||
           launch_grad_matern_if<29>(a, s) ||
           launch_grad_matern_if<30>(a, s);
}

}  // namespace nngp
