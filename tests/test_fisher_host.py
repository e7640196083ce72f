"""Fisher information sweep, host side (no GPU): the restatement of tests/fisher_ref.py pinned by its second form
and by the dense GP, its fp64 conditioning on the GPU tests' field, the Fisher-scoring iteration on a quadratic,
and the C entry point's and the Python methods' refusals before any HIP call.
"""
import numpy as np
import pytest

import fisher_ref as R
from pynngp_amd import _lib, fisher

M_ALL = tuple(range(1, 33))


@pytest.fixture(scope="module")
def field96():
    coords, y = R.field(96, seed=1)
    return coords, y, {m: R.knn_prior(coords, m) for m in M_ALL}


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("kind", R.KINDS)
def test_two_forms_agree_per_row(field96, kind):
    coords, _, sets = field96
    th = R.theta_of(kind)
    worst = 0.0
    for m in (1, 2, 8, 9, 15, 16, 23, 24, 31, 32):
        a = R.rows_bf(coords, sets[m], kind, th)["I"]
        b = R.rows_trace(coords, sets[m], kind, th)
        worst = max(worst, float(np.max(np.abs(a - b) / (1 + np.abs(b)))))
    print(kind, "max |I_bf - I_trace| / (1 + |I|) =", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("kind", R.KINDS)
def test_row_sum_is_the_dense_information(kind):
    coords, _ = R.field(40, seed=1)
    th = R.theta_of(kind)
    s = R.rows_bf(coords, R.full_sets(40), kind, th)["I"].sum(0)
    dense = R.dense_info(coords, kind, th)
    print(kind, "rel err", np.max(np.abs(s - dense) / np.abs(dense)))
    assert np.allclose(s, dense, rtol=1e-10, atol=0)


@pytest.mark.skipif(not R.HAVE_EXTENDED, reason="np.longdouble is not an extended format here")
@pytest.mark.parametrize("kind", R.KINDS)
def test_fp64_restatement_against_longdouble_twin(field96, kind):
    """The conditioning of the inputs: the fp64 restatement within 1e-11 (1 + |I|) of its extended-precision twin
    for every m, which makes the GPU tests' 1e-9 a statement about the kernel."""
    coords, y, sets = field96
    th = R.theta_of(kind)
    worst = 0.0
    for m in M_ALL:
        a = R.rows_bf(coords, sets[m], kind, th, y)
        b = R.rows_bf(coords, sets[m], kind, th, y, dtype=np.longdouble)
        for key in ("I", "G"):
            worst = max(worst, float(np.max(np.abs(a[key] - b[key]) / (1 + np.abs(b[key])))))
    print(kind, "max |fp64 - longdouble| / (1 + |ref|) =", worst)
    assert worst <= 1e-11


def test_gradient_rows_match_the_gradient_sweeps_formulas(field96):
    """G of the (dF, W) form equals bf_grad's (dF, dr) form (test_gpu_grad.py's restatement, restated here)."""
    coords, y, sets = field96
    kind, th = "matern32", R.theta_of("matern32")
    nbr = sets[10]
    got = R.rows_bf(coords, nbr, kind, th, y)["G"]
    C, dC, idx, ok = R.blocks(coords, nbr, kind, th, np.float64)
    for i in (0, 3, 50, 95):
        k = int(ok[i, :-1].sum())
        sel = list(range(k)) + [10]
        Ci = C[i][np.ix_(sel, sel)]
        yy = y[idx[i, sel]]
        Ni = np.linalg.inv(Ci[:k, :k])
        b, a = Ni @ Ci[:k, k], Ni @ yy[:k]
        u, al = np.append(-b, 1.0), np.append(a, 0.0)
        F, r = u @ Ci @ u, yy[k] - b @ yy[:k]
        for j in range(3):
            dCj = dC[j][i][np.ix_(sel, sel)]
            ref = -0.5 * ((u @ dCj @ u / F) * (1 - r * r / F) + 2 * r * (-(al @ dCj @ u)) / F)
            assert abs(got[i, j] - ref) <= 1e-11 * (1 + abs(ref))


# ---------------------------------------------------------------- Fisher scoring on a toy
def test_scoring_on_a_quadratic_converges_in_one_step():
    A = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.2], [0.5, 0.2, 2.0]])
    zs = np.array([0.3, -1.2, 2.0])

    def evaluate(z):
        d = z - zs
        return -0.5 * d @ A @ d, -A @ d, A

    res = fisher.fisher_scoring(evaluate, [0.0, 0.0, 0.0])
    assert res["converged"] and res["n_iter"] == 1 and res["ridge"] == 0.0
    assert np.allclose(res["z"], zs, atol=1e-12)


def test_scoring_halves_an_overlong_step_and_counts():
    """An information 10 times too small: the full step overshoots (the likelihood falls), halvings recover."""
    A = np.diag([2.0, 5.0])
    zs = np.array([1.0, -1.0])
    trials = []

    def evaluate(z):
        d = z - zs
        return -0.5 * d @ A @ d, -A @ d, A / 10.0

    def ll_only(z):
        trials.append(np.array(z))
        d = z - zs
        return -0.5 * d @ A @ d

    res = fisher.fisher_scoring(evaluate, [0.0, 0.0], loglik_only=ll_only, tol=1e-12, maxiter=200)
    assert res["converged"] and np.allclose(res["z"], zs, atol=1e-5)
    assert res["n_loglik_evals"] == len(trials) > res["n_iter"] >= 1  # some step was halved


def test_scoring_stops_at_maxiter_and_on_failure():
    def evaluate(z):
        return -float(z[0] ** 4), np.array([-4.0 * z[0] ** 3]), np.array([[1e3]])  # tiny steps: slow

    res = fisher.fisher_scoring(evaluate, [1.0], maxiter=3)
    assert not res["converged"] and res["n_iter"] == 3
    with pytest.raises(FloatingPointError):
        fisher.fisher_scoring(lambda z: None, [0.0])


def test_ridge_rule():
    g = np.array([1.0, 1.0])
    step, ridge = fisher.scoring_step(np.array([[4.0, 1.0], [1.0, 9.0]]), g)
    assert ridge == 0.0 and np.allclose(np.array([[4.0, 1.0], [1.0, 9.0]]) @ step, g)
    sing = np.array([[1.0, 2.0], [2.0, 4.0]])  # unit-diagonal form [[1, 1], [1, 1]]: eigenvalues 0 and 2
    step, ridge = fisher.scoring_step(sing, g)
    assert abs(ridge - 2.0 * fisher.RIDGE_RCOND) <= 1e-15 and np.all(np.isfinite(step))
    step, ridge = fisher.scoring_step(np.array([[2.0, 0.0], [0.0, 0.0]]), np.array([1.0, 0.0]))  # a dead parameter
    assert np.allclose(step, [0.5, 0.0])


def test_matrix_helpers():
    v = np.arange(1.0, 7.0)
    I = fisher.info_matrix(v)
    assert np.array_equal(I, I.T) and np.array_equal(I[np.triu_indices(3)], v)
    th = np.array([2.0, 3.0, 5.0])
    Il, gl = fisher.to_log(I, np.ones(3), th)
    assert np.allclose(Il, np.diag(th) @ I @ np.diag(th)) and np.array_equal(gl, th)
    assert np.allclose(fisher.info_matrix(fisher.info_rows_scale(v[None], th))[0], Il)
    P = np.array([[4.0, 1.0], [1.0, 3.0]])
    cov, se = fisher.theta_cov(P)
    assert np.allclose(cov, np.linalg.inv(P)) and np.allclose(se, np.sqrt(np.diag(np.linalg.inv(P))))


# ---------------------------------------------------------------- refusals before any HIP call
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _codes():
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nngp.h")).read()
    return {name: int(re.search(r"#define\s+" + name + r"\s+\(?(-?\d+)", hdr).group(1))
            for name in ("NNGP_OK", "NNGP_EINVAL", "NNGP_EUNSUP")}


def _call(lib, *, coords=256, n_points=100, dim=2, nbr=512, order=None, n_rows=100, m=10, i0=0, kind=0,
          theta=(1.0, 6.0, 0.1), values=768, I_rows=None, G=None, partials=1024, grad=1280, info=1536, workspace=4096,
          ws_bytes=None):
    # fake (never dereferenced) device addresses: every refusal below happens before any HIP call
    if ws_bytes is None:
        ws_bytes = lib.nngp_bf_fisher_workspace_bytes(n_rows, m) or 4096
    return lib.nngp_bf_fisher(coords, n_points, dim, nbr, order, n_rows, m, i0, kind, *theta, values, I_rows, G,
                              partials, grad, info, workspace, ws_bytes, None)


def test_workspace_bytes(lib):
    prev = 0
    for n in (0, 1, 63, 64, 65, 1000, 10**6, 10**7):
        for m in (1, 8, 9, 32):
            assert lib.nngp_bf_fisher_workspace_bytes(n, m) % 256 == 0
        b = lib.nngp_bf_fisher_workspace_bytes(n, 15)
        assert b >= prev and b > 0
        prev = b
    for n, m in ((100, 0), (100, 33), (-1, 10)):
        assert lib.nngp_bf_fisher_workspace_bytes(n, m) == 0


def test_unsupported(lib):
    c = _codes()
    assert _call(lib, kind=5) == c["NNGP_EUNSUP"]
    assert b"matern" in lib.nngp_last_error()
    assert _call(lib, m=0, ws_bytes=4096) == c["NNGP_EUNSUP"]
    assert _call(lib, m=33, ws_bytes=4096) == c["NNGP_EUNSUP"]
    assert _call(lib, dim=4) == c["NNGP_EUNSUP"]


@pytest.mark.parametrize("kw", [
    dict(partials=None), dict(grad=None), dict(info=None), dict(coords=None), dict(workspace=None), dict(nbr=None),
    dict(ws_bytes=255), dict(workspace=4097), dict(kind=-1), dict(kind=6), dict(n_rows=-1, ws_bytes=4096),
    dict(i0=-1), dict(i0=1), dict(n_points=0), dict(theta=(0.0, 6.0, 0.1)), dict(theta=(1.0, -1.0, 0.1)),
    dict(theta=(1.0, 6.0, -0.1)), dict(theta=(float("nan"), 6.0, 0.1)), dict(theta=(1.0, float("inf"), 0.1)),
    dict(I_rows=2048, G=2048),
])
def test_invalid(lib, kw):
    assert _call(lib, **kw) == _codes()["NNGP_EINVAL"], lib.nngp_last_error()


def test_python_refusals():
    import torch

    c = torch.zeros((4, 2), dtype=torch.float64)
    nbr = torch.zeros((4, 2), dtype=torch.int32)
    with pytest.raises(_lib.NNGPExtensionError):  # CPU tensors
        _lib.bf_fisher(c, nbr, 0, "exponential", 1.0, 1.0, 0.1, None)
    with pytest.raises(ValueError):
        _lib.bf_fisher(c, nbr, 0, "exponential", 1.0, 1.0, 0.1, torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError):
        _lib.bf_fisher(c, nbr.to(torch.int64), 0, "exponential", 1.0, 1.0, 0.1, None)
    with pytest.raises(NotImplementedError):
        _lib.bf_fisher(c, nbr, 0, "matern", 1.0, 1.0, 0.1, None)
    with pytest.raises(NotImplementedError):
        _lib.bf_fisher(c, torch.zeros((4, 33), dtype=torch.int32), 0, "exponential", 1.0, 1.0, 0.1, None)
