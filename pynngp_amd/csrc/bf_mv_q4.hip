// bf_mv<4, NT> for NT = 1..4 tile rows of neighbours (bf_mv.h)
#include "bf_mv.h"

namespace nngp {

bool bf_mv_launch_q4(const MvArgs& a, hipStream_t s) {
    return launch_mv_if<4, 1>(a, s) || launch_mv_if<4, 2>(a, s) || launch_mv_if<4, 3>(a, s) ||
           launch_mv_if<4, 4>(a, s);
}

}  // namespace nngp
