// Instantiations of bf_fisher (bf_fisher.h) for m = 13..16.
#include "bf_fisher.h"

namespace nngp {

bool bf_fisher_launch_c(const FisherArgs& a, hipStream_t s) {
    return launch_fisher_if<13>(a, s) ||
           launch_fisher_if<14>(a, s) ||
           launch_fisher_if<15>(a, s) ||
           launch_fisher_if<16>(a, s);
}

}  // namespace nngp
