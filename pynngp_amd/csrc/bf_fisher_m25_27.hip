// Instantiations of bf_fisher (bf_fisher.h) for m = 25..27.
#include "bf_fisher.h"

namespace nngp {

bool bf_fisher_launch_f(const FisherArgs& a, hipStream_t s) {
    return launch_fisher_if<25>(a, s) ||
           launch_fisher_if<26>(a, s) ||
           launch_fisher_if<27>(a, s);
}

}  // namespace nngp
