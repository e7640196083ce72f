// bf_mv_grad<4, NT> for NT = 1..4 tile rows of neighbours (bf_mv_grad.h)
#include "bf_mv_grad.h"

namespace nngp {

bool bf_mv_grad_launch_q4(const MvGradArgs& a, hipStream_t s) {
    return launch_mv_grad_if<4, 1>(a, s) || launch_mv_grad_if<4, 2>(a, s) || launch_mv_grad_if<4, 3>(a, s) ||
           launch_mv_grad_if<4, 4>(a, s);
}

}  // namespace nngp
