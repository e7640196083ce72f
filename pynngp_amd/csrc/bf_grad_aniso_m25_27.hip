// Instantiations of bf_grad_aniso (bf_grad_aniso.h) for m = 25..27.
#include "bf_grad_aniso.h"

namespace nngp {

bool bf_grad_aniso_launch_f(const GradAnisoArgs& a, hipStream_t s) {
    return launch_grad_aniso_if<25>(a, s) ||
           launch_grad_aniso_if<26>(a, s) ||
           launch_grad_aniso_if<27>(a, s);
}

}  // namespace nngp
