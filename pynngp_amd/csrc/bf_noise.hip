// Per-point noise sweeps (bf_noise.h): dispatch over the instantiation units and the fixed-order folds of the
// per-block records -- bf_finalize's for the forward sweep, bf_grad's for the gradient.
#include "bf_noise.h"

namespace nngp {

hipError_t bf_noise_launch(const NoiseArgs& a, double* partials, double* grad, hipStream_t s) {
    const bool g = grad != nullptr;
    int64_t nb = 0;
    if (a.n_rows > 0) {
        nb = bf_grad_blocks(a.n_rows, a.m);
        if (!(bf_noise_launch_a(a, g, s) || bf_noise_launch_b(a, g, s) || bf_noise_launch_c(a, g, s) ||
              bf_noise_launch_d(a, g, s) || bf_noise_launch_e(a, g, s) || bf_noise_launch_f(a, g, s) ||
              bf_noise_launch_g(a, g, s) || bf_noise_launch_h(a, g, s)))
            return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return g ? bf_grad_fold_launch(a.rec, nb, partials, grad, s) : bf_finalize_launch(a.rec, nb, partials, s);
}

}  // namespace nngp
