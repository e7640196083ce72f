// Instantiations of bf_gneiting (bf_gneiting.h), forward and gradient, for m = 1..8.
#include "bf_gneiting.h"

namespace nngp {

bool bf_gneiting_launch_a(const GneitingArgs& a, bool grad, hipStream_t s) {
    return launch_gneiting_if<1>(a, grad, s) ||
           launch_gneiting_if<2>(a, grad, s) ||
           launch_gneiting_if<3>(a, grad, s) ||
           launch_gneiting_if<4>(a, grad, s) ||
           launch_gneiting_if<5>(a, grad, s) ||
           launch_gneiting_if<6>(a, grad, s) ||
           launch_gneiting_if<7>(a, grad, s) ||
           launch_gneiting_if<8>(a, grad, s);
}

}  // namespace nngp
