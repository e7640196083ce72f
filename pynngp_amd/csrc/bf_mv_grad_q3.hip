// bf_mv_grad<3, NT> for NT = 1..4 tile rows of neighbours (bf_mv_grad.h)
#include "bf_mv_grad.h"

namespace nngp {

bool bf_mv_grad_launch_q3(const MvGradArgs& a, hipStream_t s) {
    return launch_mv_grad_if<3, 1>(a, s) || launch_mv_grad_if<3, 2>(a, s) || launch_mv_grad_if<3, 3>(a, s) ||
           launch_mv_grad_if<3, 4>(a, s);
}

}  // namespace nngp
