"""The nonstationary sweeps on the GPU: nngp_bf_sweep_ns / nngp_bf_cross_ns against the long-double restatement
tests/ns_ref.py (pinned on the CPU by tests/test_ns_host.py), the torch operators, and NonstationaryNNGP.

Bounds.  Rows: bf_precision_ref.check_sweep (BF_K U scale per row on the resolved rows, the scales with the row's
largest diagonal entry).  The log-likelihood: 1e-11 relative.
"""
import numpy as np
import pytest
import torch

import het_ref as H
import ns_ref as NS
from bf_precision_ref import RESOLVED_SHARE, check_sweep
from oracle import nngp_oracle as O
from pynngp_amd import NonstationaryCovariance, NonstationaryNNGP, _lib, load_ops

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared inputs are read-only


def host(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def sweep(coords, nbr, kind, f, y, order=None, workspace=None):
    return host(*_lib.bf_sweep_ns(dev(coords), nbr if torch.is_tensor(nbr) else dev(nbr), 0, kind,
                                  tuple(dev(a) for a in f), values=dev(y), order=order, want_r=True,
                                  workspace=workspace))


def check(ref, B, F, R, p, where):
    assert ref.resolved.mean() >= RESOLVED_SHARE, (where, ref.resolved.mean())
    check_sweep(ref, B, F, R, p, where)
    ll, want = -0.5 * (len(F) * NS.LOG_2PI + p[0] + p[1]), float(ref.ll.sum())
    assert abs(ll - want) <= 1e-11 * abs(want), (where, ll, want)


@pytest.mark.parametrize("dim,kind,m", NS.CASES)
def test_sweep_matches_restatement(dim, kind, m):
    """Row by row; the first m rows carry -1 padding.  The torch operator gives the same bits."""
    coords, y, f, _, _ = NS.field(dim)
    nbr = NS.neighbours(dim, m)
    B, F, R, p = sweep(coords, nbr, kind, f, y)
    check(NS.reference(dim, m, kind), B, F, R, p, f"sweep d{dim} {kind} m{m}")
    ops = load_ops()
    Bt, Ft, Rt, pt = host(*torch.ops.nngp.bf_sweep_ns(dev(coords), dev(nbr), None, 0, ops.kind_code(kind),
                                                       *(dev(a) for a in f), dev(y), True))
    assert all(np.array_equal(a, b) for a, b in ((B, Bt), (F, Ft), (R, Rt), (p, pt)))


def test_partials_do_not_depend_on_order_or_run():
    coords, y, f, _, _ = NS.field(2)
    nbr = NS.neighbours(2, 17)
    B, F, R, p = sweep(coords, nbr, "matern32", f, y)
    perm = np.random.default_rng(3).permutation(NS.N).astype(np.int32)
    B2, F2, R2, p2 = sweep(coords, np.ascontiguousarray(nbr[perm]), "matern32", f, y, order=dev(perm))
    # again, with the smallest workspace the C ABI takes (the per-point records then live in stream-ordered memory)
    small = _lib._workspace(_lib.load().nngp_bf_sweep_ns_workspace_bytes(NS.N, 17), torch.device("cuda", 0))
    B3, F3, R3, p3 = sweep(coords, nbr, "matern32", f, y, workspace=small)
    for got in ((B2, F2, R2, p2), (B3, F3, R3, p3)):
        assert all(np.array_equal(a, b) for a, b in zip((B, F, R, p), got))


@pytest.mark.parametrize("m", [15, 17])
def test_constant_fields_agree_with_the_noise_sweep(m):
    coords, y, _, _, _ = NS.field(2)
    nbr, th, one = NS.neighbours(2, m), H.theta_of("matern52"), np.ones(NS.N)
    ref = H.rows(coords, coords, nbr, "matern52", th, y, y, one, one)
    check(ref, *sweep(coords, nbr, "matern52", [np.full(NS.N, t) for t in th], y), f"constant fields m{m}")
    Bn, Fn, Rn, pn = host(*_lib.bf_sweep_noise(dev(coords), dev(nbr), 0, "matern52", *th, dev(one), values=dev(y),
                                               want_r=True))
    check_sweep(ref, Bn, Fn, Rn, pn, f"bf_sweep_noise m{m}")


@pytest.mark.parametrize("dim,kind,m", NS.CROSS_CASES)
def test_cross_matches_restatement_and_predict_follows(dim, kind, m):
    coords, y, f, q, fq = NS.field(dim)
    nbr = NS.neighbours(dim, m, True)
    ref = NS.reference(dim, m, kind, True)
    B, F, R, p = host(*_lib.bf_cross_ns(dev(coords), dev(q), dev(nbr), kind, tuple(dev(a) for a in f),
                                        tuple(dev(a) for a in fq), ref_values=dev(y), want_r=True))
    check(ref, B, F, R, p, f"cross d{dim} {kind} m{m}")
    ops = load_ops()
    Bt, Ft, mt = host(*torch.ops.nngp.bf_cross_ns(dev(coords), dev(q), dev(nbr), ops.kind_code(kind),
                                                  *(dev(a) for a in f), *(dev(a) for a in fq), dev(y)))
    assert np.array_equal(B, Bt) and np.array_equal(F, Ft) and np.array_equal(-R, mt)
    model = NonstationaryNNGP(coords, y, m, NonstationaryCovariance(kind, *f))
    assert np.array_equal(host(_lib.knn_query(dev(coords), dev(q), m))[0], nbr)  # predict searches the same sets
    mean, var = model.predict(q, NonstationaryCovariance(kind, *fq))
    assert np.array_equal(mean, -R) and np.array_equal(var, F)
    _, var0 = model.predict(q, NonstationaryCovariance(kind, *fq), noise=False)
    assert np.allclose(var0, var - fq[2], rtol=1e-12, atol=1e-14)


def test_flags():
    coords, y, f, _, _ = NS.field(2)
    nbr = NS.neighbours(2, 8)
    clean = sweep(coords, nbr, "exponential", f, y)
    touched = lambda k, nb: (nb == k).any(axis=1) | (np.arange(NS.N) == k)  # noqa: E731
    # a refused field value: the rows that hold the point report it, the others keep their bits
    phi = f[1].copy()
    phi[77] = 0.0
    B, F, R, p = sweep(coords, nbr, "exponential", (f[0], phi, f[2]), y)
    assert p[3] == nbr_first(touched(77, nbr)) and p[2] == -1
    keep = ~touched(77, nbr)
    assert np.array_equal(B[keep], clean[0][keep]) and np.array_equal(F[keep], clean[1][keep])
    # an index one past the end
    nb = nbr.copy()
    nb[121, 3] = NS.N
    B, F, R, p = sweep(coords, nb, "exponential", f, y)
    assert p[3] == 121 and p[2] == -1 and B[121, 3] == 0.0
    keep = np.arange(NS.N) != 121
    assert np.array_equal(B[keep], clean[0][keep]) and np.array_equal(F[keep], clean[1][keep])
    # two coincident points with equal fields and no nugget: every block that holds both is singular
    c2 = coords.copy()
    c2[50] = c2[49]
    f2 = NS.fields_at(c2)
    f2[2][49] = f2[2][50] = 0.0
    nb2 = O.c_knn_prior(c2, 5)
    B, F, R, p = sweep(c2, nb2, "exponential", f2, y)
    bad = int(p[2])
    assert bad >= 50 and p[3] == -1
    assert np.isnan(F[bad]) and np.all(np.isnan(B[bad])) and np.isnan(R[bad])
    assert np.all(np.isfinite(F[:50])) and np.all(np.isfinite(F[~touched(50, nb2)]))


def nbr_first(mask):
    return int(np.nonzero(mask)[0][0])


def test_fit_recovers_a_variance_trend():
    """n = 600 in 2-D, exponential, m = 10, drawn by simulate() at log sigma2 = -0.5 + 1.5 x, phi = 8, tau2 = 0.05."""
    rng = np.random.default_rng(17)
    t = rng.uniform(0.0, 1.0, (600, 2))
    Z = np.stack([np.ones(600), t[:, 0]], axis=1)
    truth = NonstationaryCovariance("exponential", np.exp(Z @ np.array([-0.5, 1.5])), 8.0, 0.05)
    y = NonstationaryNNGP(t, np.zeros(600), 10, truth).simulate(seed=4)[0]
    flat = NonstationaryCovariance("exponential", 1.0, 5.0, 0.1)
    model = NonstationaryNNGP(t, y, 10, flat)
    ll_true = model.loglik(truth)
    res = model.fit(Z_sigma2=Z)
    stationary = NonstationaryNNGP(t, y, 10, flat).fit()
    print(f"loglik: truth {ll_true:.6f}, fit {res['loglik']:.6f} (alpha {res['alpha']}, {res['n_evals']} evaluations), "
          f"stationary {stationary['loglik']:.6f}")
    assert res["loglik"] >= ll_true - 1e-6
    assert res["alpha"][1] > 0
    assert stationary["loglik"] < res["loglik"]
    assert abs(model.loglik() - res["loglik"]) <= 1e-9 * abs(res["loglik"])
