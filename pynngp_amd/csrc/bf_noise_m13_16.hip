// Instantiations of bf_noise (bf_noise.h), forward and gradient, for m = 13..16.
#include "bf_noise.h"

namespace nngp {

bool bf_noise_launch_c(const NoiseArgs& a, bool grad, hipStream_t s) {
    return launch_noise_if<13>(a, grad, s) ||
           launch_noise_if<14>(a, grad, s) ||
           launch_noise_if<15>(a, grad, s) ||
           launch_noise_if<16>(a, grad, s);
}

}  // namespace nngp
