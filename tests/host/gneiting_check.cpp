// Host check of the Gneiting time-lag routine (pynngp_amd/csrc/gneiting_math.h with NNGP_MATH_HOST) against
// long double: 1 / psi, L = ln psi and s2 = psi^-beta over x in {0, 2^-60 .. 2^40}, the table seams
// (psi = 2^k (1 + j/128)) with their neighbours, and the seam of the direct branch (x = 2^-7).
// Prints "name value" pairs: the worst error of each output in ulp, whether x = 0 is exact, and whether the
// committed table (gneiting_table.h) agrees with log2l.
#define NNGP_MATH_HOST
#include "../../pynngp_amd/csrc/gneiting_math.h"

#include <stdio.h>

static double etab[NNGP_EXP_TAB_N], ltab[3 * NNGP_GN_TAB_N];
static double worst[3];

static double ulps(double got, long double want) {
    if (want == 0.0L) return got == 0.0 ? 0.0 : 1e30;
    int ex;
    frexpl(want, &ex);
    return (double)fabsl(((long double)got - want) / ldexpl(1.0L, ex - 53));
}

static void check(double x, double beta) {
    const CovParams Pb = nngp_gn_beta_params(beta);
    const NngpGnPsi o = nngp_gn_psi(Pb, etab, ltab, x);
    const long double L = log1pl((long double)x);
    const double e[3] = {ulps(o.ipsi, 1.0L / (1.0L + (long double)x)), ulps(o.L, L),
                         ulps(o.s2, expl(-(long double)beta * L))};
    for (int k = 0; k < 3; ++k) worst[k] = fmax(worst[k], e[k]);
}

int main() {
    nngp_exp_table_load(etab, 1.0);
    nngp_gn_table_load(ltab);
    const double betas[4] = {0.0, 0.3, 0.5, 1.0};
    uint64_t s = 0x9e3779b97f4a7c15ull;
    for (int b = 0; b < 4; ++b) {
        check(0.0, betas[b]);
        for (int ex = -60; ex <= 40; ++ex) {
            for (int i = 0; i < 2000; ++i) {  // random mantissas in the octave
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                check(ldexp(1.0 + (double)(s >> 11) * 0x1p-53, ex), betas[b]);
            }
            check(ldexp(1.0, ex), betas[b]);
            check(nextafter(ldexp(1.0, ex), 0.0), betas[b]);
        }
        for (int k = 0; k <= 40; ++k)  // psi at every table seam of every octave, one step either side
            for (int j = 0; j < NNGP_GN_TAB_N; ++j) {
                const double psi = ldexp(1.0 + j / 128.0, k);
                const double xs[3] = {nextafter(psi, 0.0) - 1.0, psi - 1.0, nextafter(psi, 1e300) - 1.0};
                for (int t = 0; t < 3; ++t)
                    if (xs[t] >= 0.0) check(xs[t], betas[b]);
            }
        check(nextafter(0x1p-7, 0.0), betas[b]);
        check(0x1p-7, betas[b]);
    }
    int table = 1;  // the committed table against long double: 1 / c_j correctly rounded, hi_j on the 2^-40 grid
    for (int j = 0; j < NNGP_GN_TAB_N; ++j) {
        const long double c = 1.0L + j / 128.0L, t = log2l(c);
        const double hi = ltab[3 * j + 1], lo = ltab[3 * j + 2];
        table &= ltab[3 * j] == (double)(1.0L / c) && ldexp(hi, 40) == rint(ldexp(hi, 40)) &&
                 fabsl((long double)hi + lo - t) <= 0x1p-62L && fabs(lo) <= 0x1p-41;
    }
    const CovParams Pb = nngp_gn_beta_params(0.5);
    const NngpGnPsi z = nngp_gn_psi(Pb, etab, ltab, 0.0), big = nngp_gn_psi(Pb, etab, ltab, 1e300);
    const int special = z.ipsi == 1.0 && z.L == 0.0 && z.s2 == 1.0 && big.s2 >= 0x1p-400 && big.ipsi > 0.0 &&
                        isfinite(big.L);
    printf("ipsi_ulp %.3f\nlog_ulp %.3f\ns2_ulp %.3f\nspecial %d\ntable %d\n", worst[0], worst[1], worst[2], special, table);
    return 0;
}
