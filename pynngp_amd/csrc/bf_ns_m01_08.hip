// Instantiations of bf_ns (bf_ns.h) for m = 1..8.
#include "bf_ns.h"

namespace nngp {

bool bf_ns_launch_a(const NsArgs& a, hipStream_t s) {
    return launch_ns_if<1>(a, s) ||
           launch_ns_if<2>(a, s) ||
           launch_ns_if<3>(a, s) ||
           launch_ns_if<4>(a, s) ||
           launch_ns_if<5>(a, s) ||
           launch_ns_if<6>(a, s) ||
           launch_ns_if<7>(a, s) ||
           launch_ns_if<8>(a, s);
}

}  // namespace nngp
