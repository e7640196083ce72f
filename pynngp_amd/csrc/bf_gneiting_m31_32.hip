// Instantiations of bf_gneiting (bf_gneiting.h), forward and gradient, for m = 31..32.
#include "bf_gneiting.h"

namespace nngp {

bool bf_gneiting_launch_h(const GneitingArgs& a, bool grad, hipStream_t s) {
    return launch_gneiting_if<31>(a, grad, s) ||
           launch_gneiting_if<32>(a, grad, s);
}

}  // namespace nngp
