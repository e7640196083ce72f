// Instantiations of bf_grad_aniso (bf_grad_aniso.h) for m = 28..30.
#include "bf_grad_aniso.h"

namespace nngp {

bool bf_grad_aniso_launch_g(const GradAnisoArgs& a, hipStream_t s) {
    return launch_grad_aniso_if<28>(a, s) ||
           launch_grad_aniso_if<29>(a, s) ||
           launch_grad_aniso_if<30>(a, s);
}

}  // namespace nngp
