// Multivariate (coregionalised) sweep (bf_mv.h): dispatch over the instantiation units and bf_finalize's fixed-order
// fold of the per-block records.
#include "bf_mv.h"

namespace nngp {

hipError_t bf_mv_launch(const MvArgs& a, double* partials, hipStream_t s) {
    int64_t nb = 0;
    if (a.n_rows > 0) {
        nb = mv_blocks(a.n_rows);
        if (!(bf_mv_launch_q2(a, s) || bf_mv_launch_q3(a, s) || bf_mv_launch_q4(a, s))) return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return bf_finalize_launch(a.rec, nb, partials, s);
}

}  // namespace nngp
