// Instantiations of bf_grad (bf_grad.h) for m = 28..30.
#include "bf_grad.h"

namespace nngp {

bool bf_grad_launch_g(const GradArgs& a, hipStream_t s) {
    return launch_grad_if<28>(a, s) ||
           launch_grad_if<29>(a, s) ||
           launch_grad_if<30>(a, s);
}

}  // namespace nngp
