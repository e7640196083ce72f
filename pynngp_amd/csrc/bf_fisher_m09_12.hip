// Instantiations of bf_fisher (bf_fisher.h) for m = 9..12.
#include "bf_fisher.h"

namespace nngp {

bool bf_fisher_launch_b(const FisherArgs& a, hipStream_t s) {
    return launch_fisher_if<9>(a, s) ||
           launch_fisher_if<10>(a, s) ||
           launch_fisher_if<11>(a, s) ||
           launch_fisher_if<12>(a, s);
}

}  // namespace nngp
