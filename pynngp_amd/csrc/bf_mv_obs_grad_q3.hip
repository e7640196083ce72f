// bf_mv_obs_grad<3, NTMAX> for NTMAX = 1..4 tile rows of packed neighbour rows (bf_mv_obs_grad.h)
#include "bf_mv_obs_grad.h"

namespace nngp {

bool bf_mv_obs_grad_launch_q3(const MvObsGradArgs& a, hipStream_t s) {
    return launch_mv_obs_grad_if<3, 1>(a, s) || launch_mv_obs_grad_if<3, 2>(a, s) ||
           launch_mv_obs_grad_if<3, 3>(a, s) || launch_mv_obs_grad_if<3, 4>(a, s);
}

}  // namespace nngp
