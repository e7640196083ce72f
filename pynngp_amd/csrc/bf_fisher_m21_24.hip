// Instantiations of bf_fisher (bf_fisher.h) for m = 21..24.
#include "bf_fisher.h"

namespace nngp {

bool bf_fisher_launch_e(const FisherArgs& a, hipStream_t s) {
    return launch_fisher_if<21>(a, s) ||
           launch_fisher_if<22>(a, s) ||
           launch_fisher_if<23>(a, s) ||
           launch_fisher_if<24>(a, s);
}

}  // namespace nngp
