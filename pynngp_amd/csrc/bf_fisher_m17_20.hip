// Instantiations of bf_fisher (bf_fisher.h) for m = 17..20.
#include "bf_fisher.h"

namespace nngp {

bool bf_fisher_launch_d(const FisherArgs& a, hipStream_t s) {
    return launch_fisher_if<17>(a, s) ||
           launch_fisher_if<18>(a, s) ||
           launch_fisher_if<19>(a, s) ||
           launch_fisher_if<20>(a, s);
}

}  // namespace nngp
