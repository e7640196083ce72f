// Instantiations of bf_sep (bf_sep.h), forward and gradient, for m = 25..27.
#include "bf_sep.h"

namespace nngp {

bool bf_sep_launch_f(const SepArgs& a, bool grad, hipStream_t s) {
    return launch_sep_if<25>(a, grad, s) ||
           launch_sep_if<26>(a, grad, s) ||
           launch_sep_if<27>(a, grad, s);
}

}  // namespace nngp
