// Instantiations of bf_sep (bf_sep.h), forward and gradient, for m = 17..20.
#include "bf_sep.h"

namespace nngp {

bool bf_sep_launch_d(const SepArgs& a, bool grad, hipStream_t s) {
    return launch_sep_if<17>(a, grad, s) ||
           launch_sep_if<18>(a, grad, s) ||
           launch_sep_if<19>(a, grad, s) ||
           launch_sep_if<20>(a, grad, s);
}

}  // namespace nngp
