// Instantiations of bf_noise (bf_noise.h), forward and gradient, for m = 17..20.
#include "bf_noise.h"

namespace nngp {

bool bf_noise_launch_d(const NoiseArgs& a, bool grad, hipStream_t s) {
    return launch_noise_if<17>(a, grad, s) ||
           launch_noise_if<18>(a, grad, s) ||
           launch_noise_if<19>(a, grad, s) ||
           launch_noise_if<20>(a, grad, s);
}

}  // namespace nngp
