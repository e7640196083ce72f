// Instantiations of bf_grad_matern (bf_grad_matern.h) for m = 17..20.
#include "bf_grad_matern.h"

namespace nngp {

bool bf_grad_matern_launch_d(const GradMaternArgs& a, hipStream_t s) {
    return launch_grad_matern_if<17>(a, s) ||
           launch_grad_matern_if<18>(a, s) ||
           launch_grad_matern_if<19>(a, s) ||
           launch_grad_matern_if<20>(a, s);
}

}  // namespace nngp
