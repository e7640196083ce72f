// Instantiations of bf_sep (bf_sep.h), forward and gradient, for m = 31..32.
#include "bf_sep.h"

namespace nngp {

bool bf_sep_launch_h(const SepArgs& a, bool grad, hipStream_t s) {
    return launch_sep_if<31>(a, grad, s) ||
           launch_sep_if<32>(a, grad, s);
}

}  // namespace nngp
