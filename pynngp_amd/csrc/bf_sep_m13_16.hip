// Instantiations of bf_sep (bf_sep.h), forward and gradient, for m = 13..16.
#include "bf_sep.h"

namespace nngp {

bool bf_sep_launch_c(const SepArgs& a, bool grad, hipStream_t s) {
    return launch_sep_if<13>(a, grad, s) ||
           launch_sep_if<14>(a, grad, s) ||
           launch_sep_if<15>(a, grad, s) ||
           launch_sep_if<16>(a, grad, s);
}

}  // namespace nngp
