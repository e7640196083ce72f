// Binomial latent posterior (latent_binomial.hip): the Newton step's link kernel (d, rhs, g per node and the
// fixed-order fold of its block records into partials[4]) and the logistic-normal integral.  Included by that
// unit and the C ABI only, like latent.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nngp {

size_t binomial_newton_step_workspace_bytes(int64_t n);
hipError_t binomial_newton_step_launch(int64_t n, const int32_t* trials, const double* successes,
                                       const double* offset, const double* w, double* d, double* rhs, double* g,
                                       double* partials, void* workspace, hipStream_t s);
hipError_t logistic_normal_launch(int64_t n, const double* mu, const double* sd, double* out, hipStream_t s);

}  // namespace nngp
