// bf_mv_obs_grad<2, NTMAX> for NTMAX = 1..4 tile rows of packed neighbour rows (bf_mv_obs_grad.h)
#include "bf_mv_obs_grad.h"

namespace nngp {

bool bf_mv_obs_grad_launch_q2(const MvObsGradArgs& a, hipStream_t s) {
    return launch_mv_obs_grad_if<2, 1>(a, s) || launch_mv_obs_grad_if<2, 2>(a, s) ||
           launch_mv_obs_grad_if<2, 3>(a, s) || launch_mv_obs_grad_if<2, 4>(a, s);
}

}  // namespace nngp
