// Instantiations of bf_fisher (bf_fisher.h) for m = 1..8.
#include "bf_fisher.h"

namespace nngp {

bool bf_fisher_launch_a(const FisherArgs& a, hipStream_t s) {
    return launch_fisher_if<1>(a, s) ||
           launch_fisher_if<2>(a, s) ||
           launch_fisher_if<3>(a, s) ||
           launch_fisher_if<4>(a, s) ||
           launch_fisher_if<5>(a, s) ||
           launch_fisher_if<6>(a, s) ||
           launch_fisher_if<7>(a, s) ||
           launch_fisher_if<8>(a, s);
}

}  // namespace nngp
