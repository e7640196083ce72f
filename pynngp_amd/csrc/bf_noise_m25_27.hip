// Instantiations of bf_noise (bf_noise.h), forward and gradient, for m = 25..27.
#include "bf_noise.h"

namespace nngp {

bool bf_noise_launch_f(const NoiseArgs& a, bool grad, hipStream_t s) {
    return launch_noise_if<25>(a, grad, s) ||
           launch_noise_if<26>(a, grad, s) ||
           launch_noise_if<27>(a, grad, s);
}

}  // namespace nngp
