// Instantiations of bf_grad_matern (bf_grad_matern.h) for m = 1..8.
#include "bf_grad_matern.h"

namespace nngp {

bool bf_grad_matern_launch_a(const GradMaternArgs& a, hipStream_t s) {
    return launch_grad_matern_if<1>(a, s) ||
           launch_grad_matern_if<2>(a, s) ||
           launch_grad_matern_if<3>(a, s) ||
           launch_grad_matern_if<4>(a, s) ||
           launch_grad_matern_if<5>(a, s) ||
           launch_grad_matern_if<6>(a, s) ||
           launch_grad_matern_if<7>(a, s) ||
           launch_grad_matern_if<8>(a, s);
}

}  // namespace nngp
