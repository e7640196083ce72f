// Instantiations of bf_noise (bf_noise.h), forward and gradient, for m = 1..8.
#include "bf_noise.h"

namespace nngp {

bool bf_noise_launch_a(const NoiseArgs& a, bool grad, hipStream_t s) {
    return launch_noise_if<1>(a, grad, s) ||
           launch_noise_if<2>(a, grad, s) ||
           launch_noise_if<3>(a, grad, s) ||
           launch_noise_if<4>(a, grad, s) ||
           launch_noise_if<5>(a, grad, s) ||
           launch_noise_if<6>(a, grad, s) ||
           launch_noise_if<7>(a, grad, s) ||
           launch_noise_if<8>(a, grad, s);
}

}  // namespace nngp
