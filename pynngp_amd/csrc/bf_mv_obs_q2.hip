// bf_mv_obs<2, NTMAX> for NTMAX = 1..4 tile rows of packed neighbour rows (bf_mv_obs.h)
#include "bf_mv_obs.h"

namespace nngp {

bool bf_mv_obs_launch_q2(const MvObsArgs& a, hipStream_t s) {
    return launch_mv_obs_if<2, 1>(a, s) || launch_mv_obs_if<2, 2>(a, s) || launch_mv_obs_if<2, 3>(a, s) ||
           launch_mv_obs_if<2, 4>(a, s);
}

}  // namespace nngp
