// Instantiations of bf_grad_matern (bf_grad_matern.h) for m = 31..32.
#include "bf_grad_matern.h"

namespace nngp {

bool bf_grad_matern_launch_h(const GradMaternArgs& a, hipStream_t s) {
    return launch_grad_matern_if<31>(a, s) ||
           launch_grad_matern_if<32>(a, s);
}

}  // namespace nngp
