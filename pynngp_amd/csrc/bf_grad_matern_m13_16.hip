// Instantiations of bf_grad_matern (bf_grad_matern.h) for m = 13..16.
#include "bf_grad_matern.h"

namespace nngp {

bool bf_grad_matern_launch_c(const GradMaternArgs& a, hipStream_t s) {
    return launch_grad_matern_if<13>(a, s) ||
           launch_grad_matern_if<14>(a, s) ||
           launch_grad_matern_if<15>(a, s) ||
           launch_grad_matern_if<16>(a, s);
}

}  // namespace nngp
