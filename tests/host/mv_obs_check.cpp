// Stand-alone check of the host side of the packed-row multivariate sweep (pynngp_amd/csrc/mv_obs_host.h): scope, tile
// count, workspace size and the argument checks of nngp_bf_sweep_mv_obs / nngp_bf_cross_mv_obs, meant to be built with
// -fsanitize=address,undefined.  Prints "ok" and the workspace size of (n_rows, m, q) = (1001, 50, 2), which
// tests/test_mv_obs_host.py compares.
#include <cstdio>
#include <vector>

#include "mv_obs_host.h"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

int main() {
    using namespace nngp;
    CHECK(mv_obs_tiles(1) == 1 && mv_obs_tiles(16) == 1 && mv_obs_tiles(17) == 2 && mv_obs_tiles(64) == 4);
    CHECK(mv_obs_workspace_bytes(10, 64, 2) == 0 && mv_obs_workspace_bytes(10, 0, 2) == 0);
    CHECK(mv_obs_workspace_bytes(10, 5, 1) == 0 && mv_obs_workspace_bytes(10, 5, 5) == 0);
    CHECK(mv_obs_workspace_bytes(-1, 5, 2) == 0 && mv_obs_workspace_bytes(((int64_t)1 << 47) + 1, 5, 2) == 0);
    // a record per location: never smaller than bf_mv's record per block, which mv_obs_check relies on
    for (int q = kMvMinQ; q <= kMvMaxQ; ++q)
        for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)9, (int64_t)1000003, (int64_t)1 << 47}) {
            const size_t b = mv_obs_workspace_bytes(n, kMvObsMaxM, q);
            CHECK(b > 0 && b % 256 == 0 && b >= (size_t)(n > 0 ? n : 1) * 4 * sizeof(double));
            CHECK(b >= mv_workspace_bytes(n, 1, q));
        }
    for (int q = kMvMinQ; q <= kMvMaxQ; ++q) {
        std::vector<double> A(q * q, 0.0), phi(q, 2.0), tau2(q, 0.0);
        for (int a = 0; a < q; ++a)
            for (int b = 0; b <= a; ++b) A[a * q + b] = a == b ? 1.0 : -0.5;
        std::vector<unsigned char> raw(mv_obs_workspace_bytes(8, kMvObsMaxM, q) + 256);
        void* ws = (void*)(((uintptr_t)raw.data() + 255) & ~(uintptr_t)255);
        double coords[8] = {0}, partials[4];
        int32_t nbr[8 * 63];
        uint8_t obs[8] = {0};
        MvError e;
        auto call = [&](int m, int qq, int kind, int c, const void* o, int rows_max, size_t bytes) {
            return mv_obs_check(e, coords, 8, 1, nbr, 8, m, qq, 0, 8, kind, A.data(), phi.data(), tau2.data(), c, o,
                                rows_max, partials, ws, bytes);
        };
        const size_t full = raw.size() - 256;
        CHECK(call(63, q, 0, 1, obs, 64, full) == NNGP_OK && call(1, q, 3, 8, obs, 1, full) == NNGP_OK);
        CHECK(call(64, q, 0, 1, obs, 64, full) == NNGP_EUNSUP && call(0, q, 0, 1, obs, 64, full) == NNGP_EUNSUP);
        CHECK(call(5, q, 0, 1, obs, 65, full) == NNGP_EUNSUP && call(5, q, 0, 1, obs, 0, full) == NNGP_EUNSUP);
        CHECK(call(5, 1, 0, 1, obs, 8, full) == NNGP_EUNSUP && call(5, 5, 0, 1, obs, 8, full) == NNGP_EUNSUP);
        CHECK(call(5, q, 4, 1, obs, 8, full) == NNGP_EUNSUP && call(5, q, 5, 1, obs, 8, full) == NNGP_EUNSUP);
        CHECK(call(5, q, 9, 1, obs, 8, full) == NNGP_EINVAL && call(5, q, 0, 9, obs, 8, full) == NNGP_EINVAL);
        CHECK(call(5, q, 0, 1, nullptr, 8, full) == NNGP_EINVAL && e.msg[0] != 0);
        CHECK(call(5, q, 0, 1, obs, 8, full - 256) == NNGP_EINVAL);  // bf_mv's size passes, this sweep's does not
        tau2[q - 1] = -1e-3;
        CHECK(call(5, q, 0, 1, obs, 8, full) == NNGP_EINVAL);
    }
    std::printf("ok %zu\n", mv_obs_workspace_bytes(1001, 50, 2));
    return 0;
}
