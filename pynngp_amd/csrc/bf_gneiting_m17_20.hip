// Instantiations of bf_gneiting (bf_gneiting.h), forward and gradient, for m = 17..20.
#include "bf_gneiting.h"

namespace nngp {

bool bf_gneiting_launch_d(const GneitingArgs& a, bool grad, hipStream_t s) {
    return launch_gneiting_if<17>(a, grad, s) ||
           launch_gneiting_if<18>(a, grad, s) ||
           launch_gneiting_if<19>(a, grad, s) ||
           launch_gneiting_if<20>(a, grad, s);
}

}  // namespace nngp
