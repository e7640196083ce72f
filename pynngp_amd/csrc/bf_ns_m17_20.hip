// Instantiations of bf_ns (bf_ns.h) for m = 17..20.
#include "bf_ns.h"

namespace nngp {

bool bf_ns_launch_d(const NsArgs& a, hipStream_t s) {
    return launch_ns_if<17>(a, s) ||
           launch_ns_if<18>(a, s) ||
           launch_ns_if<19>(a, s) ||
           launch_ns_if<20>(a, s);
}

}  // namespace nngp
