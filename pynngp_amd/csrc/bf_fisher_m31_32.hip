// Instantiations of bf_fisher (bf_fisher.h) for m = 31..32.
#include "bf_fisher.h"

namespace nngp {

bool bf_fisher_launch_h(const FisherArgs& a, hipStream_t s) {
    return launch_fisher_if<31>(a, s) ||
           launch_fisher_if<32>(a, s);
}

}  // namespace nngp
