"""CPU: the whitened Gram sweep's C ABI (nngp_whiten_gram) is exported, bound and documented consistently and rejects
bad arguments before any GPU call; the torch op refuses CPU tensors; and the host algebra of pynngp_amd/regression.py
(GLS, REML, the Normal-inverse-gamma posterior and the evidence from a given Gram matrix) agrees with dense numpy
formulas built from a random SPD precision at n = 40, p = 3.

The dense comparison's tolerance: every quantity is a rational function of the Gram matrix G of [y, X] under the
precision Q; both sides start from the same fp64 Q, y and X, so they differ by the rounding of two different
evaluation orders, each within a small multiple of cond(X'QX) eps relative (Higham, Accuracy and Stability, Thm 10.4
for the Cholesky solve).  The bound is 64 cond(X'QX) eps; measured (python tests/test_whiten_host.py prints them):
GLS largest relative difference 4.1e-16 (cov_beta) at cond = 3.8, bound 5.4e-14; Normal-inverse-gamma 5.2e-15 (b with
the proper prior, whose dense form goes through the n x n marginal covariance) at cond = 1.8, bound 2.5e-14.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
EPS = 2.0 ** -52
EINVAL = -1
NEW = ("nngp_whiten_gram_workspace_bytes", "nngp_whiten_gram")
ARGS = ["P", "P", "P", "P", "I64", "I32", "I64", "I64", "I32", "P", "P", "P", "P", "P", "SZ", "P"]


@pytest.fixture(scope="module")
def lib():
    from pynngp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.load()


def test_header_binding_and_document_agree(lib):
    from pynngp_amd import _lib

    ct = {ctypes.c_void_p: "P", ctypes.c_int32: "I32", ctypes.c_int64: "I64", ctypes.c_size_t: "SZ"}
    for s in NEW:
        assert s in _lib.SYMBOLS, s
        assert getattr(lib, s).argtypes is not None, s
    assert [ct[t] for t in lib.nngp_whiten_gram.argtypes] == ARGS
    assert [ct[t] for t in lib.nngp_whiten_gram_workspace_bytes.argtypes] == ["I64", "I32"]
    assert lib.nngp_whiten_gram_workspace_bytes.restype is ctypes.c_size_t
    hdr = open(os.path.join(ROOT, "include", "nngp.h")).read()
    m = re.search(r"#define\s+NNGP_WHITEN_MAX_COLS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 16 == _lib.WHITEN_MAX_COLS
    proto = re.search(r"int nngp_whiten_gram\(([^;]*)\);", hdr, flags=re.S).group(1)
    codes = []
    for a in proto.split(","):
        tok = a.replace("const", " ").split()[0]
        codes.append("P" if "*" in a else {"int64_t": "I64", "int32_t": "I32", "size_t": "SZ"}[tok])
    assert codes == ARGS
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"_lib\.nngp_whiten_gram\.argtypes\s*=\s*\[([^\]]*)\]", doc)
    assert m and [t.strip() for t in m.group(1).split(",")] == ARGS
    assert "_lib.nngp_whiten_gram_workspace_bytes.argtypes = [I64, I32]" in doc
    assert lib.nngp_abi_version() == 4 and _lib.ABI_VERSION == 4  # a pure addition


P = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731

# fake non-null, 256-byte aligned "device" addresses: every refusal below must come before any launch
WG = dict(nbr=256, order=None, B=512, F=768, n_rows=50, m=5, i0=0, n_points=50, ncol=3, V=1024, Vq=None, U=1280,
          gram=1536, workspace=2048, workspace_bytes=1 << 20)


def _wg(lib, **kw):
    a = dict(WG)
    a.update(kw)
    return lib.nngp_whiten_gram(P(a["nbr"]), P(a["order"]), P(a["B"]), P(a["F"]), a["n_rows"], a["m"], a["i0"],
                                a["n_points"], a["ncol"], P(a["V"]), P(a["Vq"]), P(a["U"]), P(a["gram"]),
                                P(a["workspace"]), a["workspace_bytes"], None)


@pytest.mark.parametrize("kw", [
    dict(ncol=0), dict(ncol=17), dict(U=None), dict(workspace_bytes=8), dict(m=0), dict(n_rows=-1),
    dict(m=64), dict(nbr=None), dict(B=None), dict(F=None), dict(V=None), dict(workspace=None), dict(workspace=2049),
    dict(U=1024), dict(Vq=1280), dict(i0=-1), dict(i0=1), dict(n_rows=51), dict(n_points=0), dict(n_rows=1 << 31),
])
def test_rejects_bad_arguments_before_any_launch(lib, kw):
    assert _wg(lib, **kw) == EINVAL, (kw, lib.nngp_last_error())
    assert lib.nngp_last_error()


def test_workspace_sizes(lib):
    ws = lib.nngp_whiten_gram_workspace_bytes
    for bad in ((-1, 3), (100, 0), (100, 17), (100, -1)):
        assert ws(*bad) == 0, bad
    assert ws(0, 3) > 0 and ws(0, 3) % 256 == 0
    for n, k in ((1, 1), (1000, 2), (4097, 16), (10 ** 6, 16)):
        tiles = (n + 1023) // 1024
        got = ws(n, k)
        assert got % 256 == 0 and got >= tiles * (k * (k + 1) // 2) * 8, (n, k, got)
        assert got < tiles * (k * (k + 1) // 2) * 8 + 256
    # a workspace one byte short of the stated size is refused, the stated size passes the check (and then the
    # n_rows = 0 call returns without a launch)
    need = ws(50, 3)
    assert _wg(lib, workspace_bytes=need - 1) == EINVAL


def test_zero_rows_is_ok_without_a_launch(lib):
    assert _wg(lib, n_rows=0, gram=None, workspace_bytes=lib.nngp_whiten_gram_workspace_bytes(0, 3)) == 0
    assert _wg(lib, n_rows=0, gram=None, Vq=4096, n_points=7, workspace_bytes=256) == 0


def test_torch_op_and_wrapper_refuse_cpu_tensors():
    from pynngp_amd import _lib, load_ops

    load_ops()
    assert hasattr(torch.ops.nngp, "whiten_gram")
    nbr = torch.full((6, 2), -1, dtype=torch.int32)
    B, F, V = (torch.zeros(s, dtype=torch.float64) for s in ((6, 2), (6,), (6, 3)))
    with pytest.raises(NotImplementedError):
        torch.ops.nngp.whiten_gram(nbr, None, B, F, 0, V, None, True)
    with pytest.raises(_lib.NNGPExtensionError):
        _lib.whiten_gram(nbr, B, F, V)


def test_fake_kernel_traces_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from pynngp_amd import load_ops

    load_ops()
    with FakeTensorMode():
        nbr = torch.empty((9, 4), dtype=torch.int32)
        B, F, V = (torch.empty(s, dtype=torch.float64) for s in ((9, 4), (9,), (9, 5)))
        U, G = torch.ops.nngp.whiten_gram(nbr, None, B, F, 0, V, None, True)
        assert U.shape == (9, 5) and G.shape == (5, 5)
        U, G = torch.ops.nngp.whiten_gram(nbr, None, B, F, 0, V, None, False)
        assert U.shape == (9, 5) and G.shape == (0, 0)


# ---------------------------------------------------------------- host algebra against dense numpy
def _dense_case(seed=0, n=40, p=3):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    Q = A @ A.T / n + np.eye(n)                       # a random SPD precision
    X = np.column_stack([np.ones(n), rng.standard_normal((n, p - 1))])
    y = X @ np.array([1.5, -0.7, 0.3][:p]) + rng.standard_normal(n)
    V = np.column_stack([y, X])
    G = V.T @ Q @ V
    sum_log_f = -np.linalg.slogdet(Q)[1]              # sum log F = log det C = -log det Q
    return Q, X, y, G, sum_log_f


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _gls_gaps():
    from pynngp_amd import regression as R

    Q, X, y, G, slf = _dense_case()
    n, p = X.shape
    res = R.gls_from_gram(G, slf, n)
    XQX = X.T @ Q @ X
    cond = np.linalg.cond(XQX)
    beta = np.linalg.solve(XQX, X.T @ Q @ y)
    r = y - X @ beta
    ll = -0.5 * (n * math.log(2 * math.pi) + slf + r @ Q @ r)
    reml = -0.5 * ((n - p) * math.log(2 * math.pi) + slf + r @ Q @ r + np.linalg.slogdet(XQX)[1])
    gaps = {"beta": _rel(res.beta, beta), "cov_beta": _rel(res.cov_beta, np.linalg.inv(XQX)),
            "loglik": _rel(res.loglik, ll), "reml": _rel(res.reml, reml), "quad": _rel(res.quad, r @ Q @ r)}
    return gaps, cond


def test_gls_and_reml_match_dense_formulas():
    gaps, cond = _gls_gaps()
    for k, g in gaps.items():
        assert g <= 64 * cond * EPS, (k, g, cond)


def _nig_gaps():
    from pynngp_amd import regression as R

    Q, X, y, G, slf = _dense_case(1)
    n, p = X.shape
    C = np.linalg.inv(Q)
    out = {}
    # proper prior: the evidence is the density of a multivariate t, evaluated directly
    m0, V0, a0, b0 = np.array([0.5, 0.0, -0.2]), np.diag([4.0, 2.0, 3.0]), 3.0, 2.0
    post = R.nig_from_gram(G, slf, n, dict(mu=m0, V=V0, a=a0, b=b0))
    Vs = np.linalg.inv(np.linalg.inv(V0) + X.T @ Q @ X)
    mus = Vs @ (np.linalg.inv(V0) @ m0 + X.T @ Q @ y)
    S = C + X @ V0 @ X.T                               # y ~ t_{2a}(X m0, (b/a) S)
    e = y - X @ m0
    maha = e @ np.linalg.solve(S, e)
    ev = (math.lgamma(a0 + n / 2) - math.lgamma(a0) - 0.5 * n * math.log(2 * math.pi * b0)
          - 0.5 * np.linalg.slogdet(S)[1] - (a0 + n / 2) * math.log1p(maha / (2 * b0)))
    out["proper"] = {"mu": _rel(post.mu, mus), "V": _rel(post.V, Vs), "a": abs(post.a - (a0 + n / 2)),
                     "b": _rel(post.b, b0 + 0.5 * maha), "evidence": _rel(post.log_evidence, ev)}
    # flat prior on beta: mu = GLS beta, V = (X'QX)^-1, a = a0 + (n - p) / 2, b = b0 + quad / 2
    post = R.nig_from_gram(G, slf, n, dict(a=a0, b=b0))
    XQX = X.T @ Q @ X
    beta = np.linalg.solve(XQX, X.T @ Q @ y)
    r = y - X @ beta
    a1, b1 = a0 + (n - p) / 2, b0 + 0.5 * r @ Q @ r
    ev = (-0.5 * (n - p) * math.log(2 * math.pi) - 0.5 * slf - 0.5 * np.linalg.slogdet(XQX)[1] + a0 * math.log(b0)
          - a1 * math.log(b1) + math.lgamma(a1) - math.lgamma(a0))
    out["flat"] = {"mu": _rel(post.mu, beta), "V": _rel(post.V, np.linalg.inv(XQX)), "a": abs(post.a - a1),
                   "b": _rel(post.b, b1), "evidence": _rel(post.log_evidence, ev)}
    return out, np.linalg.cond(XQX)


def test_nig_posterior_and_evidence_match_dense_formulas():
    out, cond = _nig_gaps()
    for prior, gaps in out.items():
        for k, g in gaps.items():
            assert g <= 64 * cond * EPS, (prior, k, g, cond)


def test_rank_deficient_design_raises():
    from pynngp_amd import NNGPNumericalError
    from pynngp_amd import regression as R

    Q, X, y, _, slf = _dense_case()
    X = np.column_stack([X, X[:, 1] - 2.0 * X[:, 2]])
    V = np.column_stack([y, X])
    with pytest.raises(NNGPNumericalError):
        R.gls_from_gram(V.T @ Q @ V, slf, X.shape[0])
    with pytest.raises(NNGPNumericalError):
        R.nig_from_gram(V.T @ Q @ V, slf, X.shape[0])


if __name__ == "__main__":
    print(_gls_gaps())
    print(_nig_gaps())
