// bf_mv<2, NT> for NT = 1..4 tile rows of neighbours (bf_mv.h)
#include "bf_mv.h"

namespace nngp {

bool bf_mv_launch_q2(const MvArgs& a, hipStream_t s) {
    return launch_mv_if<2, 1>(a, s) || launch_mv_if<2, 2>(a, s) || launch_mv_if<2, 3>(a, s) ||
           launch_mv_if<2, 4>(a, s);
}

}  // namespace nngp
