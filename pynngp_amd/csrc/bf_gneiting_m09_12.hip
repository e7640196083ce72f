// Instantiations of bf_gneiting (bf_gneiting.h), forward and gradient, for m = 9..12.
#include "bf_gneiting.h"

namespace nngp {

bool bf_gneiting_launch_b(const GneitingArgs& a, bool grad, hipStream_t s) {
    return launch_gneiting_if<9>(a, grad, s) ||
           launch_gneiting_if<10>(a, grad, s) ||
           launch_gneiting_if<11>(a, grad, s) ||
           launch_gneiting_if<12>(a, grad, s);
}

}  // namespace nngp
