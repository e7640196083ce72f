"""``pynngp_amd.loglik``: the NNGP log-likelihood as a differentiable torch function of theta (and values)."""
import math

import torch

from . import _lib

_KINDS = ("exponential", "matern32", "matern52", "gaussian", "spherical")


class _LogLik(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coords, nbr, theta, values, kind, order):
        from . import load_ops

        load_ops()
        th = [float(x) for x in theta.detach().cpu().tolist()]  # host synchronisation (the flags are the other)
        p, g, _ = torch.ops.nngp.bf_grad(coords, nbr, order, 0, _lib.KIND_CODES[kind], th[0], th[1], th[2],
                                         values.detach(), False)
        ctx.save_for_backward(coords, nbr, values, g)
        ctx.meta = (kind, order, th, theta.device)
        ctx.mark_non_differentiable(p)
        ll = -0.5 * (nbr.shape[0] * math.log(2.0 * math.pi) + p[0] + p[1])
        return ll, p

    @staticmethod
    def backward(ctx, grad_out, _grad_p):
        coords, nbr, values, g = ctx.saved_tensors
        kind, order, th, tdev = ctx.meta
        gtheta = (grad_out * g).to(tdev) if ctx.needs_input_grad[2] else None
        gvalues = None
        if ctx.needs_input_grad[3]:
            # d l / d y = -(I - B)^T (r / F): one ordinary sweep (B, F, R) and torch indexing, not hot-path work
            rows, m = nbr.shape
            R = torch.empty(rows, dtype=torch.float64, device=coords.device)
            B, F, _ = _lib.bf_sweep(coords, nbr, 0, kind, th[0], th[1], th[2], values=values.detach(), order=order, R=R)
            w = R / F
            nat = nbr if order is None else torch.empty_like(nbr).index_copy_(0, order.long(), nbr)
            gvalues = -w
            ok = nat >= 0
            gvalues = gvalues.index_add(0, nat.clamp(min=0).long().reshape(-1), (B * w[:, None] * ok).reshape(-1))
            gvalues = grad_out * gvalues
        return None, None, gtheta, gvalues, None, None


class _LogLikAniso(torch.autograd.Function):
    """theta = (sigma2, phi_1 .. phi_dim, tau2): the per-axis sweep (``torch.ops.nngp.bf_grad_aniso``)."""

    @staticmethod
    def forward(ctx, coords, nbr, theta, values, kind, order):
        from . import load_ops

        load_ops()
        th = [float(x) for x in theta.detach().cpu().tolist()]  # host synchronisation (the flags are the other)
        p, g, _ = torch.ops.nngp.bf_grad_aniso(coords, nbr, order, 0, _lib.KIND_CODES[kind], th[0], th[1:-1], th[-1],
                                               values.detach(), False)
        ctx.save_for_backward(coords, nbr, values, g)
        ctx.meta = (kind, order, th, theta.device)
        ctx.mark_non_differentiable(p)
        ll = -0.5 * (nbr.shape[0] * math.log(2.0 * math.pi) + p[0] + p[1])
        return ll, p

    @staticmethod
    def backward(ctx, grad_out, _grad_p):
        coords, nbr, values, g = ctx.saved_tensors
        kind, order, th, tdev = ctx.meta
        gtheta = (grad_out * g).to(tdev) if ctx.needs_input_grad[2] else None
        gvalues = None
        if ctx.needs_input_grad[3]:
            # as _LogLik: one ordinary sweep, at phi = 1 on the coordinates scaled column by column
            rows, m = nbr.shape
            scaled = coords * torch.tensor(th[1:-1], dtype=torch.float64, device=coords.device)
            R = torch.empty(rows, dtype=torch.float64, device=coords.device)
            B, F, _ = _lib.bf_sweep(scaled, nbr, 0, kind, th[0], 1.0, th[-1], values=values.detach(), order=order, R=R)
            w = R / F
            nat = nbr if order is None else torch.empty_like(nbr).index_copy_(0, order.long(), nbr)
            gvalues = -w
            ok = nat >= 0
            gvalues = gvalues.index_add(0, nat.clamp(min=0).long().reshape(-1), (B * w[:, None] * ok).reshape(-1))
            gvalues = grad_out * gvalues
        return None, None, gtheta, gvalues, None, None


class _LogLikMatern(torch.autograd.Function):
    """theta = (sigma2, phi, tau2, nu): the general-nu Matern sweep (``torch.ops.nngp.bf_grad_matern``)."""

    @staticmethod
    def forward(ctx, coords, nbr, theta, values, order):
        from . import load_ops

        load_ops()
        th = [float(x) for x in theta.detach().cpu().tolist()]  # host synchronisation (the flags are the other)
        p, g, _ = torch.ops.nngp.bf_grad_matern(coords, nbr, order, 0, th[0], th[1], th[2], th[3], values.detach(),
                                                False)
        ctx.save_for_backward(coords, nbr, values, g)
        ctx.meta = (order, th, theta.device)
        ctx.mark_non_differentiable(p)
        ll = -0.5 * (nbr.shape[0] * math.log(2.0 * math.pi) + p[0] + p[1])
        return ll, p

    @staticmethod
    def backward(ctx, grad_out, _grad_p):
        coords, nbr, values, g = ctx.saved_tensors
        order, th, tdev = ctx.meta
        gtheta = (grad_out * g).to(tdev) if ctx.needs_input_grad[2] else None
        gvalues = None
        if ctx.needs_input_grad[3]:
            # as _LogLik: one ordinary sweep (B, F, R) of the matern kind at nu
            rows, m = nbr.shape
            R = torch.empty(rows, dtype=torch.float64, device=coords.device)
            B, F, _ = _lib.bf_sweep(coords, nbr, 0, "matern", th[0], th[1], th[2], values=values.detach(), order=order,
                                    R=R, nu=th[3])
            w = R / F
            nat = nbr if order is None else torch.empty_like(nbr).index_copy_(0, order.long(), nbr)
            gvalues = -w
            ok = nat >= 0
            gvalues = gvalues.index_add(0, nat.clamp(min=0).long().reshape(-1), (B * w[:, None] * ok).reshape(-1))
            gvalues = grad_out * gvalues
        return None, None, gtheta, gvalues, None


class _LogLikNoise(torch.autograd.Function):
    """Per-point noise tau2 * v (``torch.ops.nngp.bf_grad_noise``); no gradient with respect to v."""

    @staticmethod
    def forward(ctx, coords, nbr, theta, values, kind, order, v):
        from . import load_ops

        load_ops()
        th = [float(x) for x in theta.detach().cpu().tolist()]  # host synchronisation (the flags are the other)
        p, g, _ = torch.ops.nngp.bf_grad_noise(coords, nbr, order, 0, _lib.KIND_CODES[kind], th[0], th[1], th[2],
                                               values.detach(), v, False)
        ctx.save_for_backward(coords, nbr, values, g, v)
        ctx.meta = (kind, order, th, theta.device)
        ctx.mark_non_differentiable(p)
        ll = -0.5 * (nbr.shape[0] * math.log(2.0 * math.pi) + p[0] + p[1])
        return ll, p

    @staticmethod
    def backward(ctx, grad_out, _grad_p):
        coords, nbr, values, g, v = ctx.saved_tensors
        kind, order, th, tdev = ctx.meta
        gtheta = (grad_out * g).to(tdev) if ctx.needs_input_grad[2] else None
        gvalues = None
        if ctx.needs_input_grad[3]:
            # as _LogLik: one ordinary sweep (B, F, R) of the same model
            B, F, R, _ = _lib.bf_sweep_noise(coords, nbr, 0, kind, th[0], th[1], th[2], v, values=values.detach(),
                                             order=order, want_r=True)
            w = R / F
            nat = nbr if order is None else torch.empty_like(nbr).index_copy_(0, order.long(), nbr)
            gvalues = -w
            ok = nat >= 0
            gvalues = gvalues.index_add(0, nat.clamp(min=0).long().reshape(-1), (B * w[:, None] * ok).reshape(-1))
            gvalues = grad_out * gvalues
        return None, None, gtheta, gvalues, None, None, None


class _LogLikSep(torch.autograd.Function):
    """theta = (sigma2, phi_s, phi_t, tau2): the separable space-time sweep (``torch.ops.nngp.bf_grad_sep``)."""

    @staticmethod
    def forward(ctx, coords, nbr, theta, values, kind_s, kind_t, order):
        from . import load_ops

        load_ops()
        th = [float(x) for x in theta.detach().cpu().tolist()]  # host synchronisation (the flags are the other)
        p, g, _ = torch.ops.nngp.bf_grad_sep(coords, nbr, order, 0, _lib.KIND_CODES[kind_s], _lib.KIND_CODES[kind_t],
                                             th[0], th[1], th[2], th[3], values.detach(), False)
        ctx.save_for_backward(coords, nbr, values, g)
        ctx.meta = (kind_s, kind_t, order, th, theta.device)
        ctx.mark_non_differentiable(p)
        ll = -0.5 * (nbr.shape[0] * math.log(2.0 * math.pi) + p[0] + p[1])
        return ll, p

    @staticmethod
    def backward(ctx, grad_out, _grad_p):
        coords, nbr, values, g = ctx.saved_tensors
        kind_s, kind_t, order, th, tdev = ctx.meta
        gtheta = (grad_out * g).to(tdev) if ctx.needs_input_grad[2] else None
        gvalues = None
        if ctx.needs_input_grad[3]:
            # as _LogLik: one ordinary sweep (B, F, R) of the same model
            B, F, R, _ = _lib.bf_sweep_sep(coords, nbr, 0, kind_s, kind_t, th[0], th[1], th[2], th[3],
                                           values=values.detach(), order=order, want_r=True)
            w = R / F
            nat = nbr if order is None else torch.empty_like(nbr).index_copy_(0, order.long(), nbr)
            gvalues = -w
            ok = nat >= 0
            gvalues = gvalues.index_add(0, nat.clamp(min=0).long().reshape(-1), (B * w[:, None] * ok).reshape(-1))
            gvalues = grad_out * gvalues
        return None, None, gtheta, gvalues, None, None, None


def loglik_sep(coords, nbr, kind_s, kind_t, theta4, values, order=None):
    """NNGP log-likelihood of ``values`` on S = T under the separable space-time covariance
    ``sigma2 rho_s(phi_s d_s) rho_t(phi_t d_t) + tau2 delta`` (time in the last column of ``coords``, dim 2 or 3) at
    ``theta4`` = (sigma2, phi_s, phi_t, tau2), a float64 (4,) tensor, differentiable in ``theta4`` and, when
    ``values.requires_grad``, in ``values``.

    Forward runs one gradient sweep (``torch.ops.nngp.bf_grad_sep``) and synchronises with the host as
    :func:`loglik` does; backward returns ``grad_out * grad`` for theta with no further launch.  ``nbr`` (N, m) int32
    with 1 <= m <= 32; factors exponential .. spherical; the not-PD and bad-index flags raise.
    """
    for k in (kind_s, kind_t):
        if k not in _lib.KIND_CODES:
            raise ValueError(f"unknown covariance kind {k!r}")
        if k not in _KINDS:
            raise NotImplementedError(f"loglik_sep serves the factor kinds {_KINDS}")
    if theta4.dtype != torch.float64 or theta4.shape != (4,):
        raise ValueError("theta4 must be a float64 (4,) tensor (sigma2, phi_s, phi_t, tau2)")
    if coords.dim() != 2 or coords.shape[1] not in (2, 3):
        raise NotImplementedError("loglik_sep serves 2 or 3 coordinate columns (space, then time)")
    if nbr.dim() != 2 or not 1 <= nbr.shape[1] <= _lib.GRAD_MAX_M:
        raise NotImplementedError(f"loglik_sep's gradient serves 1 <= m <= {_lib.GRAD_MAX_M}")
    if nbr.shape[0] != coords.shape[0]:
        raise ValueError("loglik_sep is an S = T sweep: one nbr row per location")
    ll, p = _LogLikSep.apply(coords, nbr, theta4, values, kind_s, kind_t, order)
    from .nngp import _raise_on_bad

    _raise_on_bad(p.detach().cpu().numpy())
    return ll


class _LogLikArd(torch.autograd.Function):
    """theta = (sigma2, phi_1 .. phi_dim, tau2): the n-dimensional sweep (``torch.ops.nngp.bf_grad_nd``)."""

    @staticmethod
    def forward(ctx, coords, nbr, theta, values, kind, order):
        from . import load_ops

        load_ops()
        th = [float(x) for x in theta.detach().cpu().tolist()]  # host synchronisation (the flags are the other)
        p, g, _ = torch.ops.nngp.bf_grad_nd(coords, nbr, order, 0, _lib.KIND_CODES[kind], th[0], th[1:-1], th[-1],
                                            values.detach(), False)
        ctx.save_for_backward(coords, nbr, values, g)
        ctx.meta = (kind, order, th, theta.device)
        ctx.mark_non_differentiable(p)
        ll = -0.5 * (nbr.shape[0] * math.log(2.0 * math.pi) + p[0] + p[1])
        return ll, p

    @staticmethod
    def backward(ctx, grad_out, _grad_p):
        coords, nbr, values, g = ctx.saved_tensors
        kind, order, th, tdev = ctx.meta
        gtheta = (grad_out * g).to(tdev) if ctx.needs_input_grad[2] else None
        gvalues = None
        if ctx.needs_input_grad[3]:
            # as _LogLik: one ordinary sweep (B, F, R) of the same model
            B, F, R, _ = _lib.bf_sweep_nd(coords, nbr, 0, kind, th[0], th[1:-1], th[-1], values=values.detach(),
                                          order=order, want_r=True)
            w = R / F
            nat = nbr if order is None else torch.empty_like(nbr).index_copy_(0, order.long(), nbr)
            gvalues = -w
            ok = nat >= 0
            gvalues = gvalues.index_add(0, nat.clamp(min=0).long().reshape(-1), (B * w[:, None] * ok).reshape(-1))
            gvalues = grad_out * gvalues
        return None, None, gtheta, gvalues, None, None


def loglik_ard(coords, nbr, kind, theta, values, order=None):
    """NNGP log-likelihood of ``values`` on S = T for 4 .. 16 coordinate columns under one decay per column,
    ``sigma2 rho(sqrt(sum_k (phi_k d_k)^2)) + tau2 delta``, at ``theta`` = (sigma2, phi_1 .. phi_dim, tau2), a float64
    (dim + 2,) tensor, differentiable in ``theta`` and, when ``values.requires_grad``, in ``values``.

    Forward runs one gradient sweep (``torch.ops.nngp.bf_grad_nd``) and synchronises with the host as
    :func:`loglik` does; backward returns ``grad_out * grad`` for theta with no further launch.  ``nbr`` (N, m) int32
    with 1 <= m <= 32; kinds exponential, matern32, matern52, gaussian; the not-PD and bad-index flags raise.
    """
    if kind not in _lib.KIND_CODES:
        raise ValueError(f"unknown covariance kind {kind!r}")
    if kind not in _lib.ND_KINDS:
        raise NotImplementedError(f"loglik_ard serves the kinds {_lib.ND_KINDS}")
    if coords.dim() != 2 or not _lib.ND_MIN_DIM <= coords.shape[1] <= _lib.ND_MAX_DIM:
        raise NotImplementedError(f"loglik_ard serves {_lib.ND_MIN_DIM} .. {_lib.ND_MAX_DIM} coordinate columns")
    if theta.dtype != torch.float64 or theta.shape != (coords.shape[1] + 2,):
        raise ValueError("theta must be a float64 (dim + 2,) tensor (sigma2, phi_1 .. phi_dim, tau2)")
    if nbr.dim() != 2 or not 1 <= nbr.shape[1] <= _lib.GRAD_MAX_M:
        raise NotImplementedError(f"loglik_ard's gradient serves 1 <= m <= {_lib.GRAD_MAX_M}")
    if nbr.shape[0] != coords.shape[0]:
        raise ValueError("loglik_ard is an S = T sweep: one nbr row per location")
    ll, p = _LogLikArd.apply(coords, nbr, theta, values, kind, order)
    from .nngp import _raise_on_bad

    _raise_on_bad(p.detach().cpu().numpy())
    return ll


def loglik_matern(coords, nbr, theta, values, order=None):
    """NNGP log-likelihood of ``values`` on S = T under the general-smoothness Matern covariance at ``theta`` =
    (sigma2, phi, tau2, nu), a float64 (4,) tensor, differentiable in all four entries of ``theta`` and, when
    ``values.requires_grad``, in ``values``.

    Forward runs one gradient sweep (``torch.ops.nngp.bf_grad_matern``) and synchronises with the host as
    :func:`loglik` does; backward returns ``grad_out * grad`` for theta with no further launch.  ``nbr`` (N, m) int32
    with 1 <= m <= 32, 0 < nu <= 50; the not-PD and bad-index flags raise.
    """
    if theta.dtype != torch.float64 or theta.shape != (4,):
        raise ValueError("theta must be a float64 (4,) tensor (sigma2, phi, tau2, nu)")
    if nbr.dim() != 2 or not 1 <= nbr.shape[1] <= _lib.GRAD_MAX_M:
        raise NotImplementedError(f"loglik_matern's gradient serves 1 <= m <= {_lib.GRAD_MAX_M}")
    if nbr.shape[0] != coords.shape[0]:
        raise ValueError("loglik_matern is an S = T sweep: one nbr row per location")
    _lib._check_kind("matern", float(theta.detach()[3]))
    ll, p = _LogLikMatern.apply(coords, nbr, theta, values, order)
    from .nngp import _raise_on_bad

    _raise_on_bad(p.detach().cpu().numpy())
    return ll


def loglik(coords, nbr, theta, values, kind, order=None, noise=None):
    """NNGP log-likelihood of ``values`` on S = T at ``theta`` = (sigma2, phi, tau2), a float64 (3,) tensor,
    differentiable in ``theta`` and, when ``values.requires_grad``, in ``values``.

    ``theta`` of shape (dim + 2,) = (sigma2, phi_1 .. phi_dim, tau2) selects the covariance with one decay per axis,
    u = sqrt(sum_k (phi_k (a_k - b_k))^2), on the raw ``coords`` (``torch.ops.nngp.bf_grad_aniso``); for
    1-D coordinates (3,) is the isotropic form, which is the same model.

    Forward runs one gradient sweep (``torch.ops.nngp.bf_grad``) and synchronises with the host twice: it
    reads theta before the launch and the sweep's two flags after it.  Backward returns ``grad_out * grad`` for theta with no further launch; the gradient in
    the values costs one ordinary sweep.  ``nbr`` (N, m) int32 with 1 <= m <= 32, ``order`` as in ``bf_sweep``
    (pass the sorted rows); kinds exponential .. spherical.  The not-PD and bad-index flags raise.

    ``noise``: a float64 (N,) device tensor of per-point noise sigmas e (the reference's ``eps``): the noise variance
    of point j is ``tau2 * e_j^2`` (``torch.ops.nngp.bf_grad_noise``; the (3,) theta only).  No gradient flows to it.
    """
    if kind not in _lib.KIND_CODES:
        raise ValueError(f"unknown covariance kind {kind!r}")
    if kind not in _KINDS:
        raise NotImplementedError("loglik's gradient serves the kinds exponential .. spherical, not the general-nu "
                                  "matern kind")
    aniso = theta.dtype == torch.float64 and theta.shape != (3,) and coords.dim() == 2 \
        and theta.shape == (coords.shape[1] + 2,)
    if not aniso and (theta.dtype != torch.float64 or theta.shape != (3,)):
        raise ValueError("theta must be a float64 (3,) tensor (sigma2, phi, tau2) or (dim + 2,) "
                         "(sigma2, phi_1 .. phi_dim, tau2)")
    if nbr.dim() != 2 or not 1 <= nbr.shape[1] <= _lib.GRAD_MAX_M:
        raise NotImplementedError(f"loglik's gradient serves 1 <= m <= {_lib.GRAD_MAX_M}")
    if nbr.shape[0] != coords.shape[0]:
        raise ValueError("loglik is an S = T sweep: one nbr row per location")
    if noise is not None:
        if aniso:
            raise NotImplementedError("loglik(noise=...) serves the isotropic (3,) theta: the per-point noise sweeps "
                                      "have no per-axis form")
        if not isinstance(noise, torch.Tensor) or noise.dtype != torch.float64 or noise.shape != (coords.shape[0],):
            raise ValueError("noise must be a float64 (N,) tensor of per-point sigmas")
        e = noise.detach()
        ll, p = _LogLikNoise.apply(coords, nbr, theta, values, kind, order, e * e)
    else:
        ll, p = (_LogLikAniso if aniso else _LogLik).apply(coords, nbr, theta, values, kind, order)
    from .nngp import _raise_on_bad

    _raise_on_bad(p.detach().cpu().numpy())
    return ll
