// Instantiations of bf_ns (bf_ns.h) for m = 28..30.
#include "bf_ns.h"

namespace nngp {

bool bf_ns_launch_g(const NsArgs& a, hipStream_t s) {
    return launch_ns_if<28>(a, s) ||
           launch_ns_if<29>(a, s) ||
           launch_ns_if<30>(a, s);
}

}  // namespace nngp
