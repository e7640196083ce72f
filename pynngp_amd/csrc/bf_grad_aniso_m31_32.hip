// Instantiations of bf_grad_aniso (bf_grad_aniso.h) for m = 31..32.
#include "bf_grad_aniso.h"

namespace nngp {

bool bf_grad_aniso_launch_h(const GradAnisoArgs& a, hipStream_t s) {
    return launch_grad_aniso_if<31>(a, s) ||
           launch_grad_aniso_if<32>(a, s);
}

}  // namespace nngp
