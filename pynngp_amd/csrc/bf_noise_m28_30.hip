// Instantiations of bf_noise (bf_noise.h), forward and gradient, for m = 28..30.
#include "bf_noise.h"

namespace nngp {

bool bf_noise_launch_g(const NoiseArgs& a, bool grad, hipStream_t s) {
    return launch_noise_if<28>(a, grad, s) ||
           launch_noise_if<29>(a, grad, s) ||
           launch_noise_if<30>(a, grad, s);
}

}  // namespace nngp
