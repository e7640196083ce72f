// Instantiations of bf_ns (bf_ns.h) for m = 9..12.
#include "bf_ns.h"

namespace nngp {

bool bf_ns_launch_b(const NsArgs& a, hipStream_t s) {
    return launch_ns_if<9>(a, s) ||
           launch_ns_if<10>(a, s) ||
           launch_ns_if<11>(a, s) ||
           launch_ns_if<12>(a, s);
}

}  // namespace nngp
