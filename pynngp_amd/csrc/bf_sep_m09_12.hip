// Instantiations of bf_sep (bf_sep.h), forward and gradient, for m = 9..12.
#include "bf_sep.h"

namespace nngp {

bool bf_sep_launch_b(const SepArgs& a, bool grad, hipStream_t s) {
    return launch_sep_if<9>(a, grad, s) ||
           launch_sep_if<10>(a, grad, s) ||
           launch_sep_if<11>(a, grad, s) ||
           launch_sep_if<12>(a, grad, s);
}

}  // namespace nngp
