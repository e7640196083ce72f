// Instantiations of bf_noise (bf_noise.h), forward and gradient, for m = 9..12.
#include "bf_noise.h"

namespace nngp {

bool bf_noise_launch_b(const NoiseArgs& a, bool grad, hipStream_t s) {
    return launch_noise_if<9>(a, grad, s) ||
           launch_noise_if<10>(a, grad, s) ||
           launch_noise_if<11>(a, grad, s) ||
           launch_noise_if<12>(a, grad, s);
}

}  // namespace nngp
