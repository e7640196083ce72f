// Instantiations of bf_ns (bf_ns.h) for m = 13..16.
#include "bf_ns.h"

namespace nngp {

bool bf_ns_launch_c(const NsArgs& a, hipStream_t s) {
    return launch_ns_if<13>(a, s) ||
           launch_ns_if<14>(a, s) ||
           launch_ns_if<15>(a, s) ||
           launch_ns_if<16>(a, s);
}

}  // namespace nngp
