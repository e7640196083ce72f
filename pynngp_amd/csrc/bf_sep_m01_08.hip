// Instantiations of bf_sep (bf_sep.h), forward and gradient, for m = 1..8.
#include "bf_sep.h"

namespace nngp {

bool bf_sep_launch_a(const SepArgs& a, bool grad, hipStream_t s) {
    return launch_sep_if<1>(a, grad, s) ||
           launch_sep_if<2>(a, grad, s) ||
           launch_sep_if<3>(a, grad, s) ||
           launch_sep_if<4>(a, grad, s) ||
           launch_sep_if<5>(a, grad, s) ||
           launch_sep_if<6>(a, grad, s) ||
           launch_sep_if<7>(a, grad, s) ||
           launch_sep_if<8>(a, grad, s);
}

}  // namespace nngp
