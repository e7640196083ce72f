// Instantiations of bf_gneiting (bf_gneiting.h), forward and gradient, for m = 13..16.
#include "bf_gneiting.h"

namespace nngp {

bool bf_gneiting_launch_c(const GneitingArgs& a, bool grad, hipStream_t s) {
    return launch_gneiting_if<13>(a, grad, s) ||
           launch_gneiting_if<14>(a, grad, s) ||
           launch_gneiting_if<15>(a, grad, s) ||
           launch_gneiting_if<16>(a, grad, s);
}

}  // namespace nngp
