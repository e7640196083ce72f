// Instantiations of bf_grad_aniso (bf_grad_aniso.h) for m = 9..12.
#include "bf_grad_aniso.h"

namespace nngp {

bool bf_grad_aniso_launch_b(const GradAnisoArgs& a, hipStream_t s) {
    return launch_grad_aniso_if<9>(a, s) ||
           launch_grad_aniso_if<10>(a, s) ||
           launch_grad_aniso_if<11>(a, s) ||
           launch_grad_aniso_if<12>(a, s);
}

}  // namespace nngp
