// Instantiations of bf_grad_matern (bf_grad_matern.h) for m = 25..27.
#include "bf_grad_matern.h"

namespace nngp {

bool bf_grad_matern_launch_f(const GradMaternArgs& a, hipStream_t s) {
    return launch_grad_matern_if<25>(a, s) ||
           launch_grad_matern_if<26>(a, s) ||
           launch_grad_matern_if<27>(a, s);
}

}  // namespace nngp
