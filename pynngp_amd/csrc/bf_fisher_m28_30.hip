// Instantiations of bf_fisher (bf_fisher.h) for m = 28..30.
#include "bf_fisher.h"

namespace nngp {

bool bf_fisher_launch_g(const FisherArgs& a, hipStream_t s) {
    return launch_fisher_if<28>(a, s) ||
           launch_fisher_if<29>(a, s) ||
           launch_fisher_if<30>(a, s);
}

}  // namespace nngp
