// Instantiations of bf_grad (bf_grad.h) for m = 9..12.
#include "bf_grad.h"

namespace nngp {

bool bf_grad_launch_b(const GradArgs& a, hipStream_t s) {
    return launch_grad_if<9>(a, s) ||
           launch_grad_if<10>(a, s) ||
           launch_grad_if<11>(a, s) ||
           launch_grad_if<12>(a, s);
}

}  // namespace nngp
