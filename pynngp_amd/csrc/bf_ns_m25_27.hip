// Instantiations of bf_ns (bf_ns.h) for m = 25..27.
#include "bf_ns.h"

namespace nngp {

bool bf_ns_launch_f(const NsArgs& a, hipStream_t s) {
    return launch_ns_if<25>(a, s) ||
           launch_ns_if<26>(a, s) ||
           launch_ns_if<27>(a, s);
}

}  // namespace nngp
