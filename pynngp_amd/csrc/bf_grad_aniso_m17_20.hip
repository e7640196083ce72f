// Instantiations of bf_grad_aniso (bf_grad_aniso.h) for m = 17..20.
#include "bf_grad_aniso.h"

namespace nngp {

bool bf_grad_aniso_launch_d(const GradAnisoArgs& a, hipStream_t s) {
    return launch_grad_aniso_if<17>(a, s) ||
           launch_grad_aniso_if<18>(a, s) ||
           launch_grad_aniso_if<19>(a, s) ||
           launch_grad_aniso_if<20>(a, s);
}

}  // namespace nngp
