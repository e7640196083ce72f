// Multivariate sweep with outcomes missing at some sites (bf_mv_obs.h): dispatch over the instantiation units and
// bf_finalize's fixed-order fold of the per-location records.
#include "bf_mv_obs.h"

namespace nngp {

hipError_t bf_mv_obs_launch(const MvObsArgs& a, double* partials, hipStream_t s) {
    if (a.a.n_rows > 0) {
        if (!(bf_mv_obs_launch_q2(a, s) || bf_mv_obs_launch_q3(a, s) || bf_mv_obs_launch_q4(a, s)))
            return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return bf_finalize_launch(a.a.rec, a.a.n_rows, partials, s);
}

}  // namespace nngp
