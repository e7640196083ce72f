// Instantiations of bf_grad (bf_grad.h) for m = 13..16.
#include "bf_grad.h"

namespace nngp {

bool bf_grad_launch_c(const GradArgs& a, hipStream_t s) {
    return launch_grad_if<13>(a, s) ||
           launch_grad_if<14>(a, s) ||
           launch_grad_if<15>(a, s) ||
           launch_grad_if<16>(a, s);
}

}  // namespace nngp
