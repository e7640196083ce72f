// Instantiations of bf_gneiting (bf_gneiting.h), forward and gradient, for m = 28..30.
#include "bf_gneiting.h"

namespace nngp {

bool bf_gneiting_launch_g(const GneitingArgs& a, bool grad, hipStream_t s) {
    return launch_gneiting_if<28>(a, grad, s) ||
           launch_gneiting_if<29>(a, grad, s) ||
           launch_gneiting_if<30>(a, grad, s);
}

}  // namespace nngp
