// Instantiations of bf_grad_aniso (bf_grad_aniso.h) for m = 1..8.
#include "bf_grad_aniso.h"

namespace nngp {

bool bf_grad_aniso_launch_a(const GradAnisoArgs& a, hipStream_t s) {
    return launch_grad_aniso_if<1>(a, s) ||
           launch_grad_aniso_if<2>(a, s) ||
           launch_grad_aniso_if<3>(a, s) ||
           launch_grad_aniso_if<4>(a, s) ||
           launch_grad_aniso_if<5>(a, s) ||
           launch_grad_aniso_if<6>(a, s) ||
           launch_grad_aniso_if<7>(a, s) ||
           launch_grad_aniso_if<8>(a, s);
}

}  // namespace nngp
