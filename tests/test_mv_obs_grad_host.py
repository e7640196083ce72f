"""The packed-row multivariate gradient sweep without a GPU: the dense reference of tests/mv_obs_grad_ref.py against
central differences of the dense observed-rows log-density, and the refusals of the ctypes wrapper and the C entry
point."""
import ctypes

import numpy as np
import pytest
import torch

import mv_obs_grad_ref
from pynngp_amd import LMCCovariance, _lib

AFULL = np.array([[1.0, 0, 0], [0.5, 0.9, 0], [0.3, 0.6, 0.8]])
EINVAL, EUNSUP = -1, -4


def test_reference_against_central_differences():
    q, m, n = 3, 5, 40
    rng = np.random.default_rng(1)
    coords, Y = rng.uniform(0.0, 1.0, (n, 2)), rng.standard_normal((n, q))
    obs = 1 + (5 * np.arange(n) + 3) % 7  # a cyclic mask
    obs[7] = 0  # and a site with nothing observed
    ob = (obs[:, None] >> np.arange(q)) & 1 != 0
    Y[~ob] = np.nan
    nbr = np.full((n, m), -1, dtype=np.int32)  # prior sets: the nearest earlier points, -1 padded in the first rows
    for i in range(1, n):
        near = np.argsort(((coords[:i] - coords[i]) ** 2).sum(1))[:m]
        nbr[i, :len(near)] = near
    cov = LMCCovariance("matern32", AFULL, [3.0, 5.5, 8.0], [0.05, 0.1, 0.15])
    total = lambda c: sum(mv_obs_grad_ref.row_logdens(c, coords, nbr[i], i, Y, ob)[0] for i in range(n))  # noqa: E731
    g = mv_obs_grad_ref.reference(cov, coords, nbr, Y, ob)[2].sum(0)
    theta, low = np.array(cov.theta), np.tril_indices(q)

    def at(th):
        A = np.zeros((q, q))
        A[low] = th[:len(low[0])]
        return LMCCovariance(cov.kind, A, th[-2 * q:-q], th[-q:])

    for k in range(len(theta)):
        e = np.zeros_like(theta)
        e[k] = 1e-6 * theta[k]
        fd = (total(at(theta + e)) - total(at(theta - e))) / (2 * e[k])
        assert abs(g[k] - fd) <= 1e-6 * (1 + abs(g[k])), (k, g[k], fd)


def test_wrapper_refuses():
    def call(q=2, m=3, kind="exponential", rows_max=6):
        co, nb = torch.zeros((4, 2), dtype=torch.float64), torch.zeros((4, m), dtype=torch.int32)
        return _lib.bf_grad_mv_obs(co, nb, 0, kind, np.eye(q), (1.0,) * q, (0.0,) * q, torch.zeros(4, dtype=torch.uint8),
                                   rows_max, torch.zeros((4, q, 1), dtype=torch.float64))

    for kw in (dict(q=1), dict(q=5), dict(m=0), dict(m=64), dict(rows_max=65), dict(kind="spherical")):
        with pytest.raises(NotImplementedError):
            call(**kw)
    with pytest.raises(_lib.NNGPExtensionError):  # a valid call on CPU tensors: there is no CPU fallback
        call()


def test_entry_point_refuses_and_sizes():
    lib = _lib.load()
    raw = ctypes.create_string_buffer(8192 + 256)
    w = ctypes.c_void_p((ctypes.addressof(raw) + 255) & ~255)
    co = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)
    nb = ctypes.cast((ctypes.c_int32 * 64)(*([-1] * 64)), ctypes.c_void_p)
    p = ctypes.cast((ctypes.c_double * 32)(), ctypes.c_void_p)
    ob = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p)

    def call(m=3, q=2, kind=0, rows_max=6, obs=ob, values=co, grad=p, size=8192):
        Aa = (ctypes.c_double * 25)(*np.eye(max(q, 1)).ravel())
        ph, t2 = (ctypes.c_double * 5)(*([1.0] * 5)), (ctypes.c_double * 5)(*([0.0] * 5))
        return lib.nngp_bf_grad_mv_obs(co, 2, 2, nb, None, 1, 0, m, q, kind, Aa, ph, t2, values, obs, rows_max, None, p,
                                       grad, w, size, None)

    for kw in (dict(q=1), dict(q=5), dict(m=0), dict(m=64), dict(rows_max=0), dict(rows_max=65), dict(kind=4),
               dict(kind=5)):
        assert call(**kw) == EUNSUP, kw
    for kw in (dict(kind=8), dict(obs=None), dict(values=None), dict(grad=None), dict(size=256)):
        assert call(**kw) == EINVAL, kw
    # (4 + P) doubles per location and per chunk of 1024 locations, each part in 256-byte granules
    for m, q, npar in ((63, 2, 7), (40, 3, 12), (50, 4, 18)):
        rec = 8 * (4 + npar)
        al = lambda b: (b + 255) // 256 * 256  # noqa: E731
        assert lib.nngp_bf_grad_mv_obs_workspace_bytes(0, m, q) == 2 * al(rec)
        assert lib.nngp_bf_grad_mv_obs_workspace_bytes(3000, m, q) == al(3000 * rec) + al(3 * rec)
    for m, q in ((64, 2), (0, 3), (3, 5), (3, 1)):
        assert lib.nngp_bf_grad_mv_obs_workspace_bytes(1000, m, q) == 0
