// Instantiations of bf_sep (bf_sep.h), forward and gradient, for m = 28..30.
#include "bf_sep.h"

namespace nngp {

bool bf_sep_launch_g(const SepArgs& a, bool grad, hipStream_t s) {
    return launch_sep_if<28>(a, grad, s) ||
           launch_sep_if<29>(a, grad, s) ||
           launch_sep_if<30>(a, grad, s);
}

}  // namespace nngp
