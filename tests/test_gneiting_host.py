"""CPU: tests/gneiting_ref.py pinned by the dense density at m = n - 1 and by central differences of its own likelihood;
its fp64 twin against BF_K / 8 on the GPU test's inputs; the time-lag routine's bounds (tests/host/gneiting_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import gneiting_ref as Gn
from bf_precision_ref import BF_K, U

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", Gn.KINDS)
def test_dense_density(kind, dim):
    coords, y = Gn.field(dim, 33)
    th = Gn.theta_of(0.3)
    ref = Gn.rows(coords, coords, Gn.neighbours(dim, 32, 33), kind, th, y, y)
    want = Gn.dense_loglik(coords, kind, th, y)
    assert abs(float(ref.ll.sum()) - want) <= 1e-11 * abs(want)


@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("kind", Gn.KINDS)
def test_gradient_against_central_differences(kind, beta):
    coords, y = Gn.field(3)
    nbr = Gn.neighbours(3, 9)
    th = list(Gn.theta_of(beta))
    G = Gn.rows(coords, coords, nbr, kind, th, y, y).G.sum(0)

    def ll(t):
        return Gn.rows(coords, coords, nbr, kind, t, y, y).ll.sum()

    for k in range(5):
        # one-sided at the ends of beta's box is avoided: the restatement itself is defined outside [0, 1]
        h = Gn.LD(1e-6)
        tp, tm = [Gn.LD(v) for v in th], [Gn.LD(v) for v in th]
        tp[k], tm[k] = tp[k] + h, tm[k] - h
        fd = (ll(tp) - ll(tm)) / (2 * h)
        assert abs(float(fd - G[k])) <= 1e-8 * max(1.0, abs(float(G[k]))), (k, fd, G[k])


def twin_ratio(ref, twin):
    ok = ref.resolved
    return max((np.abs(twin.b - ref.b).max(1).astype(np.float64)[ok] / (U * ref.sB[ok])).max(),
               (np.abs(twin.F - ref.F).astype(np.float64)[ok] / (U * ref.sF[ok])).max(),
               (np.abs(twin.r - ref.r).astype(np.float64)[ok] / (U * ref.sR[ok])).max())


@pytest.mark.parametrize("dim,kind,beta,m", Gn.CASES)
def test_fp64_twin_ratio(dim, kind, beta, m):
    """The prior and the cross rows of every case the GPU test runs."""
    coords, y = Gn.field(dim)
    q, yq = Gn.query(dim)
    th = Gn.theta_of(beta)
    prior = twin_ratio(Gn.prior_reference(dim, m, kind, beta),
                       Gn.rows(coords, coords, Gn.neighbours(dim, m), kind, th, y, y, dtype=np.float64))
    cross = twin_ratio(Gn.cross_reference(dim, m, kind, beta),
                       Gn.rows(coords, q, Gn.query_neighbours(dim, m), kind, th, y, yq, dtype=np.float64))
    print(f"d{dim} {kind} beta{beta} m{m}: fp64 twin ratio prior {prior:.3g} cross {cross:.3g}")
    assert max(prior, cross) <= BF_K / 8


def test_time_lag_routine_bounds(tmp_path):
    exe = str(tmp_path / "gneiting_check")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", os.path.join(HERE, "host", "gneiting_check.cpp"),
                    "-o", exe, "-lm"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    err = {k: float(v) for k, v in zip(out[::2], out[1::2])}
    assert err["ipsi_ulp"] <= 2.0 and err["log_ulp"] <= 2.0 and err["s2_ulp"] <= 2.0, err
    assert err["special"] == 1 and err["table"] == 1
