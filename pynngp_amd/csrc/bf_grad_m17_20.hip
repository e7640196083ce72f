// Instantiations of bf_grad (bf_grad.h) for m = 17..20.
#include "bf_grad.h"

namespace nngp {

bool bf_grad_launch_d(const GradArgs& a, hipStream_t s) {
    return launch_grad_if<17>(a, s) ||
           launch_grad_if<18>(a, s) ||
           launch_grad_if<19>(a, s) ||
           launch_grad_if<20>(a, s);
}

}  // namespace nngp
