// Instantiations of bf_grad (bf_grad.h) for m = 31..32.
#include "bf_grad.h"

namespace nngp {

bool bf_grad_launch_h(const GradArgs& a, hipStream_t s) {
    return launch_grad_if<31>(a, s) ||
           launch_grad_if<32>(a, s);
}

}  // namespace nngp
