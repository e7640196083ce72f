// Instantiations of bf_noise (bf_noise.h), forward and gradient, for m = 31..32.
#include "bf_noise.h"

namespace nngp {

bool bf_noise_launch_h(const NoiseArgs& a, bool grad, hipStream_t s) {
    return launch_noise_if<31>(a, grad, s) ||
           launch_noise_if<32>(a, grad, s);
}

}  // namespace nngp
