// Stand-alone check of the host side of the 4 .. 16-dimensional path (pynngp_amd/csrc/nd_host.h): the workspace size
// and the argument checks of nngp_bf_*_nd and nngp_knn_*_nd, meant to be built with -fsanitize=address,undefined.
// Prints "ok" and the workspace size of (n_rows, m, dim) = (1000, 15, 8), which tests/test_nd_host.py compares.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nd_host.h"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

int main() {
    using namespace nngp;
    // sizes: 0 outside the scope, a positive multiple of 256 inside, enough for one record per block
    CHECK(nd_workspace_bytes(10, 15, 3) == 0 && nd_workspace_bytes(10, 15, 17) == 0);
    CHECK(nd_workspace_bytes(10, 0, 8) == 0 && nd_workspace_bytes(10, 33, 8) == 0 && nd_workspace_bytes(-1, 15, 8) == 0);
    CHECK(nd_workspace_bytes(((int64_t)1 << 47) + 1, 15, 8) == 0);
    for (int dim = kNdMinDim; dim <= kNdMaxDim; ++dim)
        for (int m = 1; m <= kNdMaxM; ++m)
            for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)255, (int64_t)256, (int64_t)1000003, (int64_t)1 << 47}) {
                const size_t b = nd_workspace_bytes(n, m, dim);
                const int64_t nb = n > 0 ? nd_blocks(n, m) : 1;
                CHECK(b > 0 && b % 256 == 0 && b >= (size_t)nb * nd_rec(dim) * sizeof(double));
                CHECK(nb * kNdThreads >= n * nd_lanes(m) && (nb - 1) * kNdThreads < (n > 0 ? n * nd_lanes(m) : 1));
            }
    CHECK(nd_rec(4) == 10 && kNdRecMax == 22);
    // the record block of the widest gradient fits what the size promises
    {
        const size_t b = nd_workspace_bytes(1000, 32, 16);
        std::vector<unsigned char> ws(b);
        const int64_t nb = nd_blocks(1000, 32);
        double* rec = reinterpret_cast<double*>(ws.data());
        for (int64_t k = 0; k < nb * nd_rec(16); ++k) rec[k] = 1.0;
        CHECK(rec[nb * nd_rec(16) - 1] == 1.0);
    }

    // argument checks: nothing but phi[0 .. dim) is dereferenced
    alignas(256) static unsigned char ws[4096];
    const double coords[8] = {0}, partials[4] = {0};
    const int32_t nbr[1] = {-1};
    std::vector<double> phi(16, 1.0);  // exactly dim entries are read: ASan sees one more
    NdError e;
    auto call = [&](int dim, int m, int kind, double s2, const double* ph, double t2, const void* c, const void* w,
                    size_t wb, int64_t rows = 1, int64_t i0 = 0) {
        return nd_sweep_check(e, c, 2, dim, nbr, rows, m, i0, 2, kind, s2, ph, t2, partials, w, wb);
    };
    CHECK(call(4, 15, NNGP_COV_EXPONENTIAL, 1.0, phi.data(), 0.1, coords, ws, sizeof ws) == NNGP_OK);
    CHECK(call(16, 32, NNGP_COV_GAUSSIAN, 1.0, phi.data(), 0.0, coords, ws, sizeof ws) == NNGP_OK);
    CHECK(call(3, 15, 0, 1.0, phi.data(), 0.1, coords, ws, sizeof ws) == NNGP_EUNSUP);
    CHECK(call(17, 15, 0, 1.0, phi.data(), 0.1, coords, ws, sizeof ws) == NNGP_EUNSUP);
    CHECK(call(8, 0, 0, 1.0, phi.data(), 0.1, coords, ws, sizeof ws) == NNGP_EUNSUP);
    CHECK(call(8, 33, 0, 1.0, phi.data(), 0.1, coords, ws, sizeof ws) == NNGP_EUNSUP);
    CHECK(call(8, 15, NNGP_COV_SPHERICAL, 1.0, phi.data(), 0.1, coords, ws, sizeof ws) == NNGP_EUNSUP);
    CHECK(std::strstr(e.msg, "positive definite") != nullptr);
    CHECK(call(8, 15, NNGP_COV_MATERN, 1.0, phi.data(), 0.1, coords, ws, sizeof ws) == NNGP_EUNSUP);
    CHECK(call(8, 15, 9, 1.0, phi.data(), 0.1, coords, ws, sizeof ws) == NNGP_EINVAL);
    CHECK(call(8, 15, 0, 1.0, nullptr, 0.1, coords, ws, sizeof ws) == NNGP_EINVAL);
    CHECK(call(8, 15, 0, 0.0, phi.data(), 0.1, coords, ws, sizeof ws) == NNGP_EINVAL);
    CHECK(call(8, 15, 0, NAN, phi.data(), 0.1, coords, ws, sizeof ws) == NNGP_EINVAL);
    CHECK(call(8, 15, 0, 1.0, phi.data(), -0.1, coords, ws, sizeof ws) == NNGP_EINVAL);
    CHECK(call(8, 15, 0, 1.0, phi.data(), INFINITY, coords, ws, sizeof ws) == NNGP_EINVAL);
    for (double bad : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
        std::vector<double> p8(8, 1.0);  // a heap array of exactly dim entries
        p8[7] = bad;
        CHECK(call(8, 15, 0, 1.0, p8.data(), 0.1, coords, ws, sizeof ws) == NNGP_EINVAL);
    }
    CHECK(call(8, 15, 0, 1.0, phi.data(), 0.1, nullptr, ws, sizeof ws) == NNGP_EINVAL);
    CHECK(call(8, 15, 0, 1.0, phi.data(), 0.1, coords, nullptr, sizeof ws) == NNGP_EINVAL);
    CHECK(call(8, 15, 0, 1.0, phi.data(), 0.1, coords, ws + 8, sizeof ws - 8) == NNGP_EINVAL);
    CHECK(call(8, 15, 0, 1.0, phi.data(), 0.1, coords, ws, 16) == NNGP_EINVAL);
    CHECK(call(8, 15, 0, 1.0, phi.data(), 0.1, coords, ws, sizeof ws, 3, 0) == NNGP_EINVAL);   // rows past the end
    CHECK(call(8, 15, 0, 1.0, phi.data(), 0.1, coords, ws, sizeof ws, 1, INT64_MAX) == NNGP_EINVAL);  // no overflow
    CHECK(call(8, 15, 0, 1.0, phi.data(), 0.1, coords, ws, sizeof ws, -1, 0) == NNGP_EINVAL);

    CHECK(nd_knn_workspace_bytes(10, 3, 5) == 0 && nd_knn_workspace_bytes(10, 17, 5) == 0);
    CHECK(nd_knn_workspace_bytes(10, 8, 33) == 0 && nd_knn_workspace_bytes(0, 8, 5) == 0);
    CHECK(nd_knn_workspace_bytes(10, 8, 5) == 256);
    CHECK(nd_knn_check(e, coords, 2, 8, 5, ws, sizeof ws) == NNGP_OK);
    CHECK(nd_knn_check(e, coords, 2, 3, 5, ws, sizeof ws) == NNGP_EUNSUP);
    CHECK(nd_knn_check(e, coords, 2, 17, 5, ws, sizeof ws) == NNGP_EUNSUP);
    CHECK(nd_knn_check(e, coords, 2, 8, 33, ws, sizeof ws) == NNGP_EUNSUP);
    CHECK(nd_knn_check(e, nullptr, 2, 8, 5, ws, sizeof ws) == NNGP_EINVAL);
    CHECK(nd_knn_check(e, coords, 2, 8, 5, nullptr, 0) == NNGP_EINVAL);
    CHECK(nd_knn_check(e, coords, 0, 8, 5, ws, sizeof ws) == NNGP_EINVAL);
    CHECK(nd_knn_check(e, coords, 2, 8, 5, ws, 8) == NNGP_EINVAL);

    std::printf("ok %zu\n", nd_workspace_bytes(1000, 15, 8));
    return 0;
}
