// Host build of the Matern-nu derivative functions of pynngp_amd/csrc/nngp_math.h (NNGP_MATH_HOST) for
// tests/test_grad_matern_host.py.  Reads "mode nu u" triples from stdin and prints "h n" as hex floats,
// h(u) = u rho'(u) and n(u) = d rho / d nu:
//   mode e: the evaluator nngp_matern_drho itself;
//   mode t: nngp_matern_tab_d over a table built as the device builder builds it (nngp_matern_table_setup,
//           the evaluator at the bins' Chebyshev nodes, nngp_matern_bin_fit_v0 with 0 in the end octaves),
//           at d2 = u^2 with the kernels' floor, phi = 1.
#define NNGP_MATH_HOST
#include "../../pynngp_amd/csrc/nngp_math.h"
#include <stdio.h>
#include <vector>

int main() {
    char mode;
    double nu, u, last_nu = -1.0;
    CovParams P{};
    bool have_tab = false;
    std::vector<double> tab;
    double costab[NNGP_MT_NC * NNGP_MT_NC];
    nngp_matern_costab(costab);
    while (scanf(" %c %lf %lf", &mode, &nu, &u) == 3) {
        if (nu != last_nu) {
            P = nngp_cov_params_nu(NNGP_KIND_MATERN, 1.0, 1.0, 0.0, nu);
            nngp_matern_table_setup(P);
            have_tab = false;
            last_nu = nu;
        }
        double h, n;
        if (mode == 'e') {
            nngp_matern_drho(P, u, &h, &n);
        } else {
            if (!have_tab) {
                tab.assign((size_t)P.mt_noct * NNGP_MT_K * 2 * NNGP_MT_NC, 0.0);
                for (int b = 0; b < P.mt_noct * NNGP_MT_K; ++b) {
                    double hv[NNGP_MT_NC], nv[NNGP_MT_NC];
                    for (int k = 0; k < NNGP_MT_NC; ++k)
                        nngp_matern_drho(P, sqrt(nngp_matern_bin_t(P, b, nngp_matern_node(k))), &hv[k], &nv[k]);
                    nngp_matern_bin_fit_v0(P, b, hv, costab, &tab[(size_t)b * 2 * NNGP_MT_NC], 0.0);
                    nngp_matern_bin_fit_v0(P, b, nv, costab, &tab[(size_t)b * 2 * NNGP_MT_NC + NNGP_MT_NC], 0.0);
                }
                have_tab = true;
            }
            nngp_matern_tab_d(P, tab.data(), fma(u, u, 0x1p-1000), &h, &n);
        }
        printf("%a %a %d %d\n", h, n, P.mt_e0, P.mt_noct);
    }
    return 0;
}
