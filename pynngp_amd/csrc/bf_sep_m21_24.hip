// Instantiations of bf_sep (bf_sep.h), forward and gradient, for m = 21..24.
#include "bf_sep.h"

namespace nngp {

bool bf_sep_launch_e(const SepArgs& a, bool grad, hipStream_t s) {
    return launch_sep_if<21>(a, grad, s) ||
           launch_sep_if<22>(a, grad, s) ||
           launch_sep_if<23>(a, grad, s) ||
           launch_sep_if<24>(a, grad, s);
}

}  // namespace nngp
