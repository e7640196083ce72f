// Instantiations of bf_ns (bf_ns.h) for m = 31..32.
#include "bf_ns.h"

namespace nngp {

bool bf_ns_launch_h(const NsArgs& a, hipStream_t s) {
    return launch_ns_if<31>(a, s) ||
           launch_ns_if<32>(a, s);
}

}  // namespace nngp
