// Instantiations of bf_grad (bf_grad.h) for m = 25..27.
#include "bf_grad.h"

namespace nngp {

bool bf_grad_launch_f(const GradArgs& a, hipStream_t s) {
    return launch_grad_if<25>(a, s) ||
           launch_grad_if<26>(a, s) ||
           launch_grad_if<27>(a, s);
}

}  // namespace nngp
