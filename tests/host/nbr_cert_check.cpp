// Host check of the neighbour-set certificate's logic (pynngp_amd/csrc/nbr_cert.h), built with
// -fsanitize=address,undefined by tests/test_cert_host.py: the checked-tile bits, the span fold, the
// theta-dependent decision, and that nngp_cov_unit without its clamp returns the clamped form's bits wherever
// the decision says "trusted".  Prints "ok" and exits 0, or the first failure and exits 1.
#define NNGP_MATH_HOST
#include "../../pynngp_amd/csrc/nbr_cert.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

using namespace nngp;

#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            printf("FAILED line %d: %s\n", __LINE__, #c);     \
            return 1;                                         \
        }                                                     \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double urand() {  // xorshift64*, [0, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) * 0x1p-53;
}

static void fill_info(int64_t* info, int64_t tiles, int64_t checked, int m, int dim, double span) {
    for (int k = 0; k < kCertInfoLen; ++k) info[k] = 0;
    info[kCertIMagic] = kCertMagic;
    info[kCertINPoints] = 1000;
    info[kCertIDim] = dim;
    info[kCertINRows] = 128 * tiles;
    info[kCertIM] = m;
    info[kCertITiles] = tiles;
    info[kCertIChecked] = checked;
    memcpy(&info[kCertISpan], &span, sizeof span);
}

template <int KIND>
static int same_bits(const int64_t* info, double span) {
    double tab[NNGP_EXP_TAB_N];
    nngp_exp_table_load_unit(tab);
    for (int trial = 0; trial < 200; ++trial) {
        const double phi = exp(log(1e-3) + urand() * (log(1e4) - log(1e-3)));
        if (cert_trusted_tiles(info, KIND, 1.0, phi, 0.0) == 0) continue;
        const CovParams P = nngp_cov_params_unit(KIND, phi, 0.0);
        for (int k = 0; k < 200; ++k) {
            // distances over the whole span, its upper end included, and tiny ones
            double d2 = k == 0 ? span : (k == 1 ? NNGP_D2_FLOOR : span * urand() * (k % 3 == 0 ? urand() * 1e-6 : 1.0));
            if (d2 < NNGP_D2_FLOOR) d2 = NNGP_D2_FLOOR;
            const double a = nngp_cov_unit<KIND, true>(P, tab, d2), b = nngp_cov_unit<KIND, false>(P, tab, d2);
            if (memcmp(&a, &b, sizeof a) != 0) {
                printf("FAILED kind %d phi %.17g d2 %.17g: %.17g vs %.17g\n", KIND, phi, d2, a, b);
                return 1;
            }
        }
    }
    return 0;
}

int main() {
    // ---- layout
    CHECK(cert_tiles(0) == 0 && cert_tiles(1) == 1 && cert_tiles(128) == 1 && cert_tiles(129) == 2);
    CHECK(cert_total_bytes(0) == 256 + (size_t)kCertSpanBlocks * 64);
    CHECK(cert_total_bytes(128 * 65) == 256 + 256 + (size_t)kCertSpanBlocks * 64);  // 65 tiles: 3 words
    CHECK(cert_mask_bytes(32 * 64 + 1) == 512);                                      // 65 words: 260 B -> 512

    // ---- checked bits: n = 300, m = 3 -> three tiles of 100 rows; row i holds min(i, m) indices
    {
        const int64_t n = 300;
        const int m = 3;
        std::vector<int32_t> nbr(n * m);
        for (int64_t i = 0; i < n; ++i)
            for (int s = 0; s < m; ++s) nbr[i * m + s] = s < i ? (int32_t)(i - 1 - s) : -1;
        std::vector<uint32_t> mask(1, 0xffffffffu);
        CHECK(cert_mask_host(nbr.data(), n, m, n, mask.data()) == 1 && mask[0] == 1u);
        nbr[150 * m + 1] = (int32_t)n;  // one past the end, in tile 1
        CHECK(cert_mask_host(nbr.data(), n, m, n, mask.data()) == 2 && mask[0] == 3u);
        nbr[150 * m + 1] = -2;
        CHECK(cert_mask_host(nbr.data(), n, m, n, mask.data()) == 2 && mask[0] == 3u);
        nbr[150 * m + 1] = 0;
        nbr[299 * m + 2] = (int32_t)(n - 1);  // the last valid index, in the last row
        CHECK(cert_mask_host(nbr.data(), n, m, n, mask.data()) == 1 && mask[0] == 1u);
        // a shard without padding: no tile checked; an empty one: nothing written past the words
        CHECK(cert_mask_host(nbr.data() + 100 * m, 200, m, n, mask.data()) == 0 && mask[0] == 0u);
        CHECK(cert_mask_host(nbr.data(), 0, m, n, mask.data()) == 0);
        // more than 32 tiles: the second word
        const int64_t big = 128 * 40;
        std::vector<int32_t> nb2(big * 2, 5);
        nb2[(128 * 33 + 7) * 2] = -1;
        std::vector<uint32_t> mask2(2, 0);
        CHECK(cert_mask_host(nb2.data(), big, 2, big, mask2.data()) == 1 && mask2[0] == 0u && mask2[1] == 2u);
    }

    // ---- span fold
    {
        std::vector<double> rec(8 * 4, 0.0);
        for (int b = 0; b < 4; ++b) {
            for (int c = 0; c < 3; ++c) {
                rec[8 * b + c] = INFINITY;  // an idle block's record
                rec[8 * b + 3 + c] = -INFINITY;
            }
        }
        rec[0] = 0.25, rec[1] = -1.0, rec[3] = 0.5, rec[4] = 0.0;
        rec[8 + 0] = 0.0, rec[8 + 1] = 0.0, rec[8 + 3] = 1.0, rec[8 + 4] = 2.0;
        double span = -1.0;
        CHECK(cert_span_fold(rec.data(), 4, 2, &span) && span == 1.0 + 9.0);
        CHECK(cert_span_fold(rec.data(), 4, 1, &span) && span == 1.0);
        rec[16 + 6] = 1.0;  // a non-finite coordinate seen by block 2
        CHECK(!cert_span_fold(rec.data(), 4, 2, &span));
        rec[16 + 6] = 0.0;
        rec[8 + 3] = 1e200;  // a finite box whose squared diagonal is not
        CHECK(!cert_span_fold(rec.data(), 4, 2, &span));
    }

    // ---- the decision
    int64_t info[kCertInfoLen];
    fill_info(info, 3, 1, 15, 2, 2.0);  // the unit square
    CHECK(cert_trusted_tiles(info, 0, 1.0, 30.0, 0.0) == 2);
    CHECK(cert_trusted_tiles(info, 0, 1.0, 1000.0, 0.0) == 0);  // phi diag log2(e) ~ 2040 > 1023
    CHECK(cert_trusted_tiles(info, 3, 1.0, 30.0, 0.0) == 0);    // gaussian: phi^2 d2 log2(e) ~ 2597
    CHECK(cert_trusted_tiles(info, 3, 1.0, 10.0, 0.0) == 2);
    CHECK(cert_trusted_tiles(info, 4, 1.0, 1000.0, 0.0) == 2);  // spherical: no clamp to bind
    CHECK(cert_trusted_tiles(info, 5, 1.0, 30.0, 0.0) == 0 && cert_trusted_tiles(info, -1, 1.0, 30.0, 0.0) == 0);
    CHECK(cert_trusted_tiles(info, 0, 0.0, 30.0, 0.0) == 0 && cert_trusted_tiles(info, 0, 1.0, NAN, 0.0) == 0);
    CHECK(cert_trusted_tiles(nullptr, 0, 1.0, 30.0, 0.0) == 0);
    info[kCertIMagic] ^= 1;
    CHECK(cert_trusted_tiles(info, 0, 1.0, 30.0, 0.0) == 0);
    fill_info(info, 3, 3, 15, 2, 2.0);
    CHECK(cert_trusted_tiles(info, 0, 1.0, 30.0, 0.0) == 0);  // every tile checked
    fill_info(info, 3, 1, 25, 2, 2.0);
    CHECK(cert_trusted_tiles(info, 0, 1.0, 30.0, 0.0) == 0);  // no trusted instance past m = 24
    // the boundary: the clamp distance itself is not trusted, a span a little inside it is
    {
        const CovParams P = nngp_cov_params_unit(0, 30.0, 0.0);
        fill_info(info, 3, 1, 15, 2, P.d2max);
        CHECK(cert_trusted_tiles(info, 0, 1.0, 30.0, 0.0) == 0);
        fill_info(info, 3, 1, 15, 2, P.d2max * (1.0 - 0x1p-30));
        CHECK(cert_trusted_tiles(info, 0, 1.0, 30.0, 0.0) == 2);
    }

    // ---- dropping the clamp changes no bit where the decision trusts
    for (double span : {2.0, 1e-6, 1e6}) {
        fill_info(info, 3, 1, 15, 2, span);
        if (same_bits<0>(info, span) || same_bits<1>(info, span) || same_bits<2>(info, span) ||
            same_bits<3>(info, span) || same_bits<4>(info, span))
            return 1;
    }
    printf("ok\n");
    return 0;
}
