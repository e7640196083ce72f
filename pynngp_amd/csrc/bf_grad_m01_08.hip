// Instantiations of bf_grad (bf_grad.h) for m = 1..8.
#include "bf_grad.h"

namespace nngp {

bool bf_grad_launch_a(const GradArgs& a, hipStream_t s) {
    return launch_grad_if<1>(a, s) ||
           launch_grad_if<2>(a, s) ||
           launch_grad_if<3>(a, s) ||
           launch_grad_if<4>(a, s) ||
           launch_grad_if<5>(a, s) ||
           launch_grad_if<6>(a, s) ||
           launch_grad_if<7>(a, s) ||
           launch_grad_if<8>(a, s);
}

}  // namespace nngp
