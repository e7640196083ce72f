// Instantiations of bf_grad_aniso (bf_grad_aniso.h) for m = 21..24.
#include "bf_grad_aniso.h"

namespace nngp {

bool bf_grad_aniso_launch_e(const GradAnisoArgs& a, hipStream_t s) {
    return launch_grad_aniso_if<21>(a, s) ||
           launch_grad_aniso_if<22>(a, s) ||
           launch_grad_aniso_if<23>(a, s) ||
           launch_grad_aniso_if<24>(a, s);
}

}  // namespace nngp
