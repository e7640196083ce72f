"""CPU: the constant and the inputs of tests/test_gpu_bf_precision.py, checked from the reference side alone.

BF_K (tests/bf_precision_ref.py) bounds |sweep - extended precision| <= BF_K U scale per row.  It is measured here from
the fp64 C oracle (``O.c_bf_sweep``, ``O.c_bf_cross``) against the np.longdouble restatement ``bf_reference``, never
from a kernel: the largest |oracle - longdouble| / (U scale) over the resolved rows of every input of the GPU file,
times 8 -- DPHI_K's margin, for the kernels' different but equally stable elimination order, fused multiply-adds and
the ~1-ulp device exp / sqrt.

Measured (``python tests/test_bf_precision_host.py`` prints them; n = 300, d = 1, 2, 3, the five kinds, m = 1 .. 32 and
33, 40, 63, easy theta on fields A and B and hard theta on field A; the cross sets at m = 5, 10, 15, 20, 28, 40; the
general-nu oracle at nu = 0.5, 1.5, 2.5 with U + EPS_NU for U):

    B 1.16 (Matern-3/2, d = 1, easy)    F 1.45 (Matern-3/2, d = 2, easy)    R 0.88 (Matern-3/2, d = 1, easy)
    cross: B 0.83, F 0.93, R 0.74       general nu: B 0.10, F 0.08, R 0.04

so BF_K = 8 x 1.45 = 11.6, rounded up to 12.  The ratios do not grow with cond(C_N): the hard thetas (cond up to 9.8e12)
stay below 1.1.  The oracle flags no row of any case, so its own precondition holds on the new inputs.

Resolved share: every (dim, m, kind, theta) case has 100 % of its rows resolved (BF_K U cond < 1) with the thetas of
bf_precision_ref.py; the largest cond is 9.8e12 (Matern-3/2, d = 1, hard).  Matern-5/2 in d = 1 runs at tau2 = 1e-9 for
that (HARD_THETAS_D1; cond up to 6.2e10).

Bite: on the easy thetas BF_K U sF / F <= 1.9e-13 and BF_K U sB / (1 + |B|) <= 1.5e-13 on every row -- 500 x and 6,000 x
tighter than the 1e-10 F and 1e-9 (1 + |B|) of the older forward tests.
"""
import numpy as np
import pytest

import bf_precision_ref as P
from oracle import nngp_oracle as O

BF_K = P.BF_K
SAMPLE_M = (1, 6, 13, 18, 24, 32)
CROSS_M = (5, 10, 15, 20, 28, 40)
wide = pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2.0 ** -60, reason="np.longdouble is no wider than fp64 here")


def prior_oracle_ratios(dim, m, kind, which, fld):
    """The oracle's worst ratios (B, F, R) on one prior-form case, and its reference."""
    theta = P.theta_of(kind, which, dim)
    coords, y = P.fields(dim)[fld], P.fields(dim)[2]
    nbr = P.neighbours(dim, m, fld)
    Bo, Fo, po = O.c_bf_sweep(coords, nbr, kind, theta, y)
    ref = P.prior_reference(dim, m, kind, theta, fld)
    assert po[2] == -1 or not ref.resolved[int(po[2])], (dim, m, kind, which, po)  # the oracle's own precondition
    return P.ratios(ref, Bo, Fo, P.oracle_residual(Bo, nbr, y, y)), ref


def cross_oracle_ratios(dim, m, kind):
    theta = P.CROSS_THETAS[kind]
    a, _, y = P.fields(dim)
    q, yq = P.cross_sets(dim)
    nbr = P.cross_neighbours(dim, m)
    Bo, Fo, po = O.c_bf_cross(a, q, nbr, kind, theta, y, yq)
    assert po[2] == -1
    ref = P.cross_reference(dim, m, kind, theta)
    return P.ratios(ref, Bo, Fo, P.oracle_residual(Bo, nbr, y, yq)), ref


def matern_oracle_ratios(dim, m, nu):
    """The general-nu oracle (a long-double integral for K_nu) against the closed form, with U + EPS_NU for U."""
    a, _, y = P.fields(dim)
    nbr = P.neighbours(dim, m, 0)
    Bo, Fo, po = O.c_bf_sweep(a, nbr, "matern", P.MATERN_THETA + (nu,), y)
    assert po[2] == -1
    ref = P.prior_reference(dim, m, P.MATERN_CLOSED[nu], P.MATERN_THETA, 0)
    return P.ratios(ref, Bo, Fo, P.oracle_residual(Bo, nbr, y, y), u=P.U + P.EPS_NU), ref


CASES = [("easy", 0), ("easy", 1), ("hard", 0)]  # (theta, field): the hard thetas on field A only


@wide
@pytest.mark.parametrize("dim", P.DIMS)
def test_bf_k_covers_fp64_against_extended_precision(dim):
    """A sample of the inputs BF_K was measured on (module docstring): 8 x the oracle's ratio stays below it; and on
    the easy thetas the bound bites: BF_K U sF / F and BF_K U sB / (1 + |B|) are at most 1e-12 on every row."""
    worst = np.zeros(3)
    for kind in P.KINDS:
        for which, fld in CASES:
            w, bite = np.zeros(3), np.zeros(2)
            for m in SAMPLE_M:
                r, ref = prior_oracle_ratios(dim, m, kind, which, fld)
                w = np.maximum(w, r)
                if which == "easy":
                    bite = np.maximum(bite, [np.max(BF_K * P.U * ref.sF / ref.F.astype(np.float64)),
                                             np.max(BF_K * P.U * ref.sB[:, None] / (1 + np.abs(ref.b.astype(np.float64))))])
            print(f"d={dim} {kind} {which} field {'AB'[fld]}: oracle ratios B {w[0]:.3g} F {w[1]:.3g} R {w[2]:.3g}"
                  + (f"; bite F {bite[0]:.3g} B {bite[1]:.3g}" if which == "easy" else ""))
            assert np.all(bite <= 1e-12), (dim, kind, fld, bite)
            worst = np.maximum(worst, w)
    for kind in ("exponential", "gaussian"):
        worst = np.maximum(worst, cross_oracle_ratios(dim, 15, kind)[0])
    worst = np.maximum(worst, matern_oracle_ratios(dim, 18, 1.5)[0])
    print(f"d={dim}: worst oracle ratios B {worst[0]:.3g} F {worst[1]:.3g} R {worst[2]:.3g}; BF_K = {BF_K:g}")
    assert 8 * worst.max() <= BF_K


@wide
@pytest.mark.parametrize("dim", P.DIMS)
def test_every_case_has_95_percent_of_its_rows_resolved(dim):
    """The cap, a condition on the inputs: every (dim, m, kind, theta, field) case of the GPU file, judged from the fp64
    eigvalsh of the long-double block alone."""
    for kind in P.KINDS:
        for which, fld in CASES:
            theta = P.theta_of(kind, which, dim)
            coords = P.fields(dim)[fld]
            low, top = 1.0, 0.0
            for m in P.M_ALL + P.M_WAVE[2:]:
                cond = P.block_cond(coords, coords, P.neighbours(dim, m, fld), kind, theta)
                share = float(np.mean(BF_K * P.U * cond < 1.0))
                assert share >= P.RESOLVED_SHARE, (dim, m, kind, which, fld, share)
                low, top = min(low, share), max(top, float(cond[np.isfinite(cond)].max()))
            print(f"d={dim} {kind} {which} field {'AB'[fld]}: resolved share >= {low:.3f}, max cond {top:.3g}")
        for m in CROSS_M:
            cond = P.block_cond(P.fields(dim)[0], P.cross_sets(dim)[0], P.cross_neighbours(dim, m), kind,
                                P.CROSS_THETAS[kind])
            assert np.all(BF_K * P.U * cond < 1.0), (dim, m, kind)


def test_reference_masks_padding_and_bad_indices_and_serves_the_cross_form():
    """-1 and out-of-range slots are decoupled (B = 0 there, the other slots as if the slot were absent); the cross
    form on the stacked coordinates is the prior form."""
    a, _, y = P.fields(2)
    nbr = np.array(P.neighbours(2, 6, 0)[:60])
    nbr[50, 2] = 10 ** 6
    theta = P.THETAS["matern32"]
    ref = P.bf_reference(a, a, nbr, "matern32", theta, y, y)
    assert np.all(ref.b[nbr < 0] == 0) and ref.b[50, 2] == 0 and ref.pad[50, 2] and ref.F[0] == np.longdouble(theta[0]) + theta[2]
    keep = [0, 1, 3, 4, 5]
    sub = P.bf_reference(a, a, nbr[:, keep], "matern32", theta, y, y)
    assert float(np.abs(ref.b[50, keep] - sub.b[50]).max()) <= 1e-17 and float(abs(ref.F[50] - sub.F[50])) <= 1e-17
    q, yq = P.cross_sets(2)
    cn = P.cross_neighbours(2, 5)
    cross = P.bf_reference(a, q, cn, "matern32", theta, y, yq)
    both = P.bf_reference(np.concatenate([a, q]), q, cn, "matern32", theta, np.concatenate([y, yq]), yq)
    assert np.array_equal(cross.b, both.b) and np.array_equal(cross.F, both.F) and np.array_equal(cross.r, both.r)
    assert (cn[:P.N_COINCIDENT, 0] >= 0).all() and np.all(a[cn[:P.N_COINCIDENT, 0]] == q[:P.N_COINCIDENT])


if __name__ == "__main__":  # the measurements quoted in the module docstring
    tot = np.zeros(3)
    for dim in P.DIMS:
        for kind in P.KINDS:
            for which, fld in CASES:
                w = np.zeros(3)
                for m in P.M_ALL + P.M_WAVE[2:]:
                    w = np.maximum(w, prior_oracle_ratios(dim, m, kind, which, fld)[0])
                print(f"d={dim} {kind} {which} {'AB'[fld]}: B {w[0]:.3g} F {w[1]:.3g} R {w[2]:.3g}", flush=True)
                tot = np.maximum(tot, w)
    print("prior form, worst (B, F, R):", tot)
    cw, mw = np.zeros(3), np.zeros(3)
    for dim in P.DIMS:
        for kind in P.KINDS:
            for m in CROSS_M:
                cw = np.maximum(cw, cross_oracle_ratios(dim, m, kind)[0])
        for m in (6, 15, 18, 24, 25, 32):
            for nu in P.MATERN_CLOSED:
                mw = np.maximum(mw, matern_oracle_ratios(dim, m, nu)[0])
    print("cross form, worst (B, F, R):", cw)
    print("general nu, worst (B, F, R):", mw)
    print("BF_K >= 8 x", max(tot.max(), cw.max(), mw.max()))
