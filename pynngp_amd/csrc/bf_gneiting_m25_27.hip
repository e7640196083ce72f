// Instantiations of bf_gneiting (bf_gneiting.h), forward and gradient, for m = 25..27.
#include "bf_gneiting.h"

namespace nngp {

bool bf_gneiting_launch_f(const GneitingArgs& a, bool grad, hipStream_t s) {
    return launch_gneiting_if<25>(a, grad, s) ||
           launch_gneiting_if<26>(a, grad, s) ||
           launch_gneiting_if<27>(a, grad, s);
}

}  // namespace nngp
