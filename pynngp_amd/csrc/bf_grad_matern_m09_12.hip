// Instantiations of bf_grad_matern (bf_grad_matern.h) for m = 9..12.
#include "bf_grad_matern.h"

namespace nngp {

bool bf_grad_matern_launch_b(const GradMaternArgs& a, hipStream_t s) {
    return launch_grad_matern_if<9>(a, s) ||
           launch_grad_matern_if<10>(a, s) ||
           launch_grad_matern_if<11>(a, s) ||
           launch_grad_matern_if<12>(a, s);
}

}  // namespace nngp
