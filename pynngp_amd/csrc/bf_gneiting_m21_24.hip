// Instantiations of bf_gneiting (bf_gneiting.h), forward and gradient, for m = 21..24.
#include "bf_gneiting.h"

namespace nngp {

bool bf_gneiting_launch_e(const GneitingArgs& a, bool grad, hipStream_t s) {
    return launch_gneiting_if<21>(a, grad, s) ||
           launch_gneiting_if<22>(a, grad, s) ||
           launch_gneiting_if<23>(a, grad, s) ||
           launch_gneiting_if<24>(a, grad, s);
}

}  // namespace nngp
