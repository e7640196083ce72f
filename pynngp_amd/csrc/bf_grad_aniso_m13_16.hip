// Instantiations of bf_grad_aniso (bf_grad_aniso.h) for m = 13..16.
#include "bf_grad_aniso.h"

namespace nngp {

bool bf_grad_aniso_launch_c(const GradAnisoArgs& a, hipStream_t s) {
    return launch_grad_aniso_if<13>(a, s) ||
           launch_grad_aniso_if<14>(a, s) ||
           launch_grad_aniso_if<15>(a, s) ||
           launch_grad_aniso_if<16>(a, s);
}

}  // namespace nngp
