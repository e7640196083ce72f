// phi-derivative sweep (bf_dphi.h): dispatch over the instantiation units and the fold of the per-block
// records into partials[4] (bf_finalize, the B/F sweep's fixed order).
#include "bf_dphi.h"

namespace nngp {

hipError_t bf_dphi_launch(const DphiArgs& a, double* partials, hipStream_t s) {
    int64_t nb = 0;
    if (a.n_rows > 0) {
        nb = bf_grad_blocks(a.n_rows, a.m);
        if (!(bf_dphi_launch_a(a, s) || bf_dphi_launch_b(a, s) || bf_dphi_launch_c(a, s) || bf_dphi_launch_d(a, s) ||
              bf_dphi_launch_e(a, s) || bf_dphi_launch_f(a, s) || bf_dphi_launch_g(a, s) || bf_dphi_launch_h(a, s)))
            return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return bf_finalize_launch(a.rec, nb, partials, s);
}

}  // namespace nngp
