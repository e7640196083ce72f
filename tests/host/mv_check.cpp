// Stand-alone check of the host side of the multivariate sweep (pynngp_amd/csrc/mv_host.h): the workspace size and
// the argument checks of nngp_bf_sweep_mv / nngp_bf_cross_mv, meant to be built with -fsanitize=address,undefined.
// Prints "ok" and the workspace size of (n_rows, m, q) = (1001, 15, 4), which tests/test_mv_host.py compares.
#include <cmath>
#include <cstdio>
#include <vector>

#include "mv_host.h"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

int main() {
    using namespace nngp;
    // sizes: 0 outside the scope, else a multiple of 256 that holds one 4-double record per block of four rows
    CHECK(mv_workspace_bytes(10, 15, 1) == 0 && mv_workspace_bytes(10, 15, 5) == 0 && mv_workspace_bytes(10, 0, 2) == 0);
    CHECK(mv_workspace_bytes(10, 32, 2) == 0 && mv_workspace_bytes(10, 21, 3) == 0 && mv_workspace_bytes(10, 16, 4) == 0);
    CHECK(mv_workspace_bytes(-1, 5, 2) == 0 && mv_workspace_bytes(((int64_t)1 << 47) + 1, 5, 2) == 0);
    for (int q = kMvMinQ; q <= kMvMaxQ; ++q)
        for (int m = 1; (m + 1) * q <= kMvMaxRows; ++m) {
            CHECK(mv_tiles(m, q) >= 1 && mv_tiles(m, q) <= 4 && 16 * mv_tiles(m, q) >= m * q);
            for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)4, (int64_t)5, (int64_t)1000003, (int64_t)1 << 47}) {
                const size_t b = mv_workspace_bytes(n, m, q);
                const int64_t nb = n > 0 ? mv_blocks(n) : 1;
                CHECK(b > 0 && b % 256 == 0 && b >= (size_t)nb * 4 * sizeof(double));
                CHECK(nb * kMvWaves >= n && (nb - 1) * kMvWaves < (n > 0 ? n : 1));
            }
        }
    // the checks read q * q, q and q doubles of exactly-sized arrays (the sanitizer watches their ends)
    for (int q = kMvMinQ; q <= kMvMaxQ; ++q) {
        std::vector<double> A(q * q, 0.0), phi(q, 2.0), tau2(q, 0.0);
        for (int a = 0; a < q; ++a)
            for (int b = 0; b <= a; ++b) A[a * q + b] = a == b ? 1.0 : -0.5;
        const int m = kMvMaxRows / q - 1;
        std::vector<unsigned char> raw(mv_workspace_bytes(8, m, q) + 256);
        void* ws = (void*)(((uintptr_t)raw.data() + 255) & ~(uintptr_t)255);
        double coords[2] = {0, 1}, partials[4];
        int32_t nbr[64];
        MvError e;
        auto call = [&](int mm, int qq, int kind, int c) {
            return mv_sweep_check(e, coords, 2, 1, nbr, 2, mm, qq, 0, 2, kind, A.data(), phi.data(), tau2.data(), c,
                                  partials, ws, raw.size() - 256);
        };
        CHECK(call(m, q, 0, 1) == NNGP_OK && call(m, q, 3, 8) == NNGP_OK);
        CHECK(call(m + 1, q, 0, 1) == NNGP_EUNSUP && call(0, q, 0, 1) == NNGP_EUNSUP);
        CHECK(call(m, q, 4, 1) == NNGP_EUNSUP && call(m, q, 5, 1) == NNGP_EUNSUP && call(m, q, 9, 1) == NNGP_EINVAL);
        CHECK(call(m, q, 0, 0) == NNGP_EINVAL && call(m, q, 0, 9) == NNGP_EINVAL);
        A[1] = 0.25;  // above the diagonal
        CHECK(call(m, q, 0, 1) == NNGP_EINVAL && e.msg[0] != 0);
        A[1] = 0.0;
        A[q * q - 1] = 0.0;
        CHECK(call(m, q, 0, 1) == NNGP_EINVAL);
        A[q * q - 1] = 1.0;
        phi[q - 1] = NAN;
        CHECK(call(m, q, 0, 1) == NNGP_EINVAL);
        phi[q - 1] = 2.0;
        tau2[q - 1] = -1e-3;
        CHECK(call(m, q, 0, 1) == NNGP_EINVAL);
        tau2[q - 1] = 0.0;
        CHECK(mv_sweep_check(e, coords, 2, 1, nbr, 3, m, q, 0, 2, 0, A.data(), phi.data(), tau2.data(), 1, partials, ws,
                             raw.size() - 256) == NNGP_EINVAL);
        CHECK(mv_sweep_check(e, coords, 2, 1, nbr, 2, m, q, 0, 2, 0, A.data(), phi.data(), tau2.data(), 1, partials, ws,
                             0) == NNGP_EINVAL);
    }
    std::printf("ok %zu\n", mv_workspace_bytes(1001, 15, 4));
    return 0;
}
