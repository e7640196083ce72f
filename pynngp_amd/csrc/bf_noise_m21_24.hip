// Instantiations of bf_noise (bf_noise.h), forward and gradient, for m = 21..24.
#include "bf_noise.h"

namespace nngp {

bool bf_noise_launch_e(const NoiseArgs& a, bool grad, hipStream_t s) {
    return launch_noise_if<21>(a, grad, s) ||
           launch_noise_if<22>(a, grad, s) ||
           launch_noise_if<23>(a, grad, s) ||
           launch_noise_if<24>(a, grad, s);
}

}  // namespace nngp
