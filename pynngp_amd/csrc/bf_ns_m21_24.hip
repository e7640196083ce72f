// Instantiations of bf_ns (bf_ns.h) for m = 21..24.
#include "bf_ns.h"

namespace nngp {

bool bf_ns_launch_e(const NsArgs& a, hipStream_t s) {
    return launch_ns_if<21>(a, s) ||
           launch_ns_if<22>(a, s) ||
           launch_ns_if<23>(a, s) ||
           launch_ns_if<24>(a, s);
}

}  // namespace nngp
