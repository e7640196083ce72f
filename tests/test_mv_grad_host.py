"""The multivariate gradient sweep without a GPU: the dense reference of tests/mv_grad_ref.py against central differences
of the dense log-densities, and the refusals of the ctypes wrapper, the operator and the C entry point."""
import ctypes

import numpy as np
import pytest
import torch

import mv_grad_ref
from pynngp_amd import LMCCovariance, _lib

AFULL = np.array([[1.0, 0, 0], [0.5, 0.9, 0], [0.3, 0.6, 0.8]])
EINVAL, EUNSUP = -1, -4


@pytest.mark.parametrize("kind", _lib.MV_KINDS)
def test_reference_against_central_differences(kind):
    q, m, n = 3, 5, 14
    rng = np.random.default_rng(1)
    coords, Y = rng.uniform(0.0, 1.0, (n, 2)), rng.standard_normal((n, q))
    nbr = np.full((n, m), -1, dtype=np.int32)  # prior sets: the nearest earlier points, -1 padded in the first rows
    for i in range(1, n):
        near = np.argsort(((coords[:i] - coords[i]) ** 2).sum(1))[:m]
        nbr[i, :len(near)] = near
    cov = LMCCovariance(kind, AFULL, [3.0, 5.5, 8.0], [0.05, 0.1, 0.15])
    total = lambda c: sum(mv_grad_ref.row_logdens(c, coords, nbr[i], i, Y)[0] for i in range(n))  # noqa: E731
    g = mv_grad_ref.reference(cov, coords, nbr, Y)[2].sum(0)
    theta, low = np.array(cov.theta), np.tril_indices(q)

    def at(th):
        A = np.zeros((q, q))
        A[low] = th[:len(low[0])]
        return LMCCovariance(kind, A, th[-2 * q:-q], th[-q:])

    for k in range(len(theta)):
        e = np.zeros_like(theta)
        e[k] = 1e-6 * theta[k]
        fd = (total(at(theta + e)) - total(at(theta - e))) / (2 * e[k])
        assert abs(g[k] - fd) <= 1e-6 * (1 + abs(g[k])), (k, g[k], fd)


def test_wrappers_refuse():
    import pynngp_amd

    co, nb = torch.zeros((4, 2), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.int32)
    vals, eye = torch.zeros((4, 2, 1), dtype=torch.float64), np.eye(2)
    with pytest.raises(_lib.NNGPExtensionError):  # a valid model on CPU tensors: there is no CPU fallback
        _lib.bf_grad_mv(co, nb, 0, "exponential", eye, (1.0, 1.0), (0.0, 0.0), vals)
    with pytest.raises(NotImplementedError):
        _lib.bf_grad_mv(co, torch.zeros((4, 32), dtype=torch.int32), 0, "exponential", eye, (1.0, 1.0), (0.0, 0.0), vals)
    with pytest.raises(NotImplementedError):
        _lib.bf_grad_mv(co, nb, 0, "spherical", eye, (1.0, 1.0), (0.0, 0.0), vals)
    with pytest.raises(ValueError):
        _lib.bf_grad_mv(co, nb, 0, "exponential", [[1.0, 0.2], [0.0, 1.0]], (1.0, 1.0), (0.0, 0.0), vals)
    with pytest.raises(ValueError):
        _lib.bf_grad_mv(co, nb, 0, "exponential", eye, (1.0, 1.0), (0.0, 0.0), vals[:, :1])
    pynngp_amd.load_ops()
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.nngp.bf_grad_mv(co, nb, None, 0, 0, [1.0, 0.0, 0.0, 1.0], [1.0, 1.0], [0.0, 0.0], vals, False)
    with pytest.raises(_lib.NNGPExtensionError):
        pynngp_amd.loglik_lmc(co, nb, "exponential", torch.eye(2, dtype=torch.float64),
                              torch.ones(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), vals[:, :, 0])


def test_entry_point_refuses_and_sizes():
    lib = _lib.load()
    raw = ctypes.create_string_buffer(8192 + 256)
    w = ctypes.c_void_p((ctypes.addressof(raw) + 255) & ~255)
    co = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)
    nb = ctypes.cast((ctypes.c_int32 * 64)(*([-1] * 64)), ctypes.c_void_p)
    p = ctypes.cast((ctypes.c_double * 32)(), ctypes.c_void_p)

    def call(m=3, q=2, kind=0, A=None, phi=None, tau2=None, values=co, grad=p, size=8192):
        Aa = (ctypes.c_double * 25)(*(np.eye(max(q, 1)).ravel() if A is None else A))
        ph = (ctypes.c_double * 5)(*([1.0] * 5 if phi is None else phi))
        t2 = (ctypes.c_double * 5)(*([0.0] * 5 if tau2 is None else tau2))
        return lib.nngp_bf_grad_mv(co, 2, 2, nb, None, 1, 0, m, q, kind, Aa, ph, t2, values, None, p, grad, w, size, None)

    for kw in (dict(q=5), dict(q=1), dict(q=2, m=32), dict(q=3, m=21), dict(q=4, m=16), dict(m=0), dict(kind=4),
               dict(kind=5)):
        assert call(**kw) == EUNSUP, kw
    for kw in (dict(A=[1.0, 0.3, 0.0, 1.0]), dict(A=[1.0, 0.0, 0.5, 0.0]), dict(phi=[1.0, 0.0]), dict(tau2=[0.0, -0.1]),
               dict(kind=8), dict(values=None), dict(grad=None), dict(size=256)):
        assert call(**kw) == EINVAL, kw
    # (4 + P) doubles per location and per chunk of 1024 locations, each part in 256-byte granules
    for m, q, npar in ((31, 2, 7), (20, 3, 12), (15, 4, 18)):
        rec = 8 * (4 + npar)
        al = lambda b: (b + 255) // 256 * 256  # noqa: E731
        assert lib.nngp_bf_grad_mv_workspace_bytes(0, m, q) == 2 * al(rec)
        assert lib.nngp_bf_grad_mv_workspace_bytes(3000, m, q) == al(3000 * rec) + al(3 * rec)
    for m, q in ((32, 2), (21, 3), (16, 4), (3, 5), (3, 1), (0, 2)):
        assert lib.nngp_bf_grad_mv_workspace_bytes(1000, m, q) == 0
