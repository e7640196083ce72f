// Multivariate gradient sweep with outcomes missing at some sites (bf_mv_obs_grad.h): dispatch over the instantiation
// units and bf_mv_grad.hip's fixed-order fold of the per-location records of 4 + P doubles (chunks of kMvGradChunk
// consecutive locations, then the chunk records in one block).
#include "bf_mv_obs_grad.h"

namespace nngp {

hipError_t bf_mv_obs_grad_launch(const MvObsGradArgs& o, double* partials, double* grad, hipStream_t s) {
    const MvGradArgs& a = o.g;
    const int nrec = 4 + mv_grad_len(a.q);
    double* crec = (double*)((char*)a.rows + mv_grad_rows_bytes(a.n_rows, a.q));
    const int64_t nc = mv_grad_chunks(a.n_rows);
    if (a.n_rows > 0) {
        if (!(bf_mv_obs_grad_launch_q2(o, s) || bf_mv_obs_grad_launch_q3(o, s) || bf_mv_obs_grad_launch_q4(o, s)))
            return hipErrorInvalidValue;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(bf_mv_grad_chunks, dim3((unsigned)nc), dim3(256), 0, s, a.rows, a.n_rows, nrec, crec);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(bf_mv_grad_finalize, dim3(1), dim3(1024), 0, s, crec, nc, nrec, partials, grad);
    return hipGetLastError();
}

}  // namespace nngp
