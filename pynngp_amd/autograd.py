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


class _LogLikGneiting(torch.autograd.Function):
    """theta = (sigma2, c, a, beta, tau2): the Gneiting space-time sweep (``torch.ops.nngp.bf_grad_gneiting``)."""

    @staticmethod
    def forward(ctx, coords, nbr, theta, values, kind, order):
        from . import load_ops

        load_ops()
        th = [float(x) for x in theta.detach().cpu().tolist()]  # host synchronisation (the flags are the other)
        p, g, _ = torch.ops.nngp.bf_grad_gneiting(coords, nbr, order, 0, _lib.KIND_CODES[kind], *th, values.detach(),
                                                  False)
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
            # as _LogLikSep: one ordinary sweep (B, F, R) of the same model
            B, F, R, _ = _lib.bf_sweep_gneiting(coords, nbr, 0, kind, *th, values=values.detach(), order=order,
                                                want_r=True)
            w = R / F
            nat = nbr if order is None else torch.empty_like(nbr).index_copy_(0, order.long(), nbr)
            ok = nat >= 0
            gvalues = (-w).index_add(0, nat.clamp(min=0).long().reshape(-1), (B * w[:, None] * ok).reshape(-1))
            gvalues = grad_out * gvalues
        return None, None, gtheta, gvalues, None, None


def loglik_gneiting(coords, nbr, kind, theta5, values, order=None):
    """NNGP log-likelihood of ``values`` on S = T under the nonseparable (Gneiting) space-time covariance
    ``sigma2 rho(c h psi^(-beta/2)) / psi + tau2 delta``, ``psi = 1 + (a u)^2`` (time in the last column of
    ``coords``, dim 2 or 3) at ``theta5`` = (sigma2, c, a, beta, tau2), a float64 (5,) tensor, differentiable in
    ``theta5`` and, when ``values.requires_grad``, in ``values``.

    Forward runs one gradient sweep (``torch.ops.nngp.bf_grad_gneiting``) and synchronises with the host as
    :func:`loglik_sep` does; backward returns ``grad_out * grad`` for theta with no further launch.  ``nbr`` (N, m)
    int32 with 1 <= m <= 32; kinds exponential, matern32, matern52, gaussian; the not-PD and bad-index flags raise.
    """
    if kind not in _lib.KIND_CODES:
        raise ValueError(f"unknown covariance kind {kind!r}")
    if kind not in _lib.GNEITING_KINDS:
        raise NotImplementedError(f"loglik_gneiting serves the kinds {_lib.GNEITING_KINDS}")
    if theta5.dtype != torch.float64 or theta5.shape != (5,):
        raise ValueError("theta5 must be a float64 (5,) tensor (sigma2, c, a, beta, tau2)")
    if coords.dim() != 2 or coords.shape[1] not in (2, 3):
        raise NotImplementedError("loglik_gneiting serves 2 or 3 coordinate columns (space, then time)")
    if nbr.dim() != 2 or not 1 <= nbr.shape[1] <= _lib.GRAD_MAX_M:
        raise NotImplementedError(f"loglik_gneiting's gradient serves 1 <= m <= {_lib.GRAD_MAX_M}")
    if nbr.shape[0] != coords.shape[0]:
        raise ValueError("loglik_gneiting is an S = T sweep: one nbr row per location")
    ll, p = _LogLikGneiting.apply(coords, nbr, theta5, values, kind, order)
    from .nngp import _raise_on_bad

    _raise_on_bad(p.detach().cpu().numpy())
    return ll


class _LogLikSvc(torch.autograd.Function):
    """theta = (sigma2_1..r, phi_1..r, tau2): the varying-coefficient sweep (``torch.ops.nngp.bf_grad_svc``)."""

    @staticmethod
    def forward(ctx, coords, Z, nbr, theta, values, kind, order):
        from . import load_ops

        load_ops()
        th = [float(x) for x in theta.detach().cpu().tolist()]  # host synchronisation (the flags are the other)
        r = (len(th) - 1) // 2
        p, g, _ = torch.ops.nngp.bf_grad_svc(coords, Z, nbr, order, 0, _lib.KIND_CODES[kind], th[:r], th[r:2 * r],
                                             th[-1], values.detach(), False)
        ctx.save_for_backward(coords, Z, nbr, values, g)
        ctx.meta = (kind, order, th, r, theta.device)
        ctx.mark_non_differentiable(p)
        ll = -0.5 * (nbr.shape[0] * math.log(2.0 * math.pi) + p[0] + p[1])
        return ll, p

    @staticmethod
    def backward(ctx, grad_out, _grad_p):
        coords, Z, nbr, values, g = ctx.saved_tensors
        kind, order, th, r, tdev = ctx.meta
        gtheta = (grad_out * g).to(tdev) if ctx.needs_input_grad[3] else None
        gvalues = None
        if ctx.needs_input_grad[4]:
            # as _LogLik: one ordinary sweep (B, F, R) of the same model
            B, F, R, _ = _lib.bf_sweep_svc(coords, Z, nbr, 0, kind, th[:r], th[r:2 * r], th[-1],
                                           values=values.detach(), order=order, want_r=True)
            w = R / F
            nat = nbr if order is None else torch.empty_like(nbr).index_copy_(0, order.long(), nbr)
            gvalues = -w
            ok = nat >= 0
            gvalues = gvalues.index_add(0, nat.clamp(min=0).long().reshape(-1), (B * w[:, None] * ok).reshape(-1))
            gvalues = grad_out * gvalues
        return None, None, None, gtheta, gvalues, None, None


def loglik_svc(coords, Z, nbr, kind, theta, values, order=None):
    """NNGP log-likelihood of ``values`` on S = T under the spatially-varying-coefficient covariance
    ``sum_k z_ak z_bk sigma2_k rho(phi_k d) + tau2 delta`` with ``Z`` (N, r) the covariates, at ``theta`` =
    (sigma2_1..r, phi_1..r, tau2), a float64 (2 r + 1,) tensor; differentiable in ``theta`` and, when
    ``values.requires_grad``, in ``values`` (not in ``Z``).

    Forward runs one gradient sweep (``torch.ops.nngp.bf_grad_svc``) and synchronises with the host as
    :func:`loglik` does; backward returns ``grad_out * grad`` for theta with no further launch.  ``nbr`` (N, m) int32
    with 1 <= m <= 32; kinds exponential .. spherical; 1 <= r <= 4; the not-PD and bad-index flags raise.
    """
    if kind not in _lib.KIND_CODES:
        raise ValueError(f"unknown covariance kind {kind!r}")
    if kind not in _lib.SVC_KINDS:
        raise NotImplementedError(f"loglik_svc serves the kinds {_lib.SVC_KINDS}")
    if Z.dim() != 2 or not 1 <= Z.shape[1] <= _lib.SVC_MAX_R:
        raise NotImplementedError(f"loglik_svc serves Z (N, r) with 1 <= r <= {_lib.SVC_MAX_R}")
    if theta.dtype != torch.float64 or theta.shape != (2 * Z.shape[1] + 1,):
        raise ValueError("theta must be a float64 (2 r + 1,) tensor (sigma2_1..r, phi_1..r, tau2)")
    if coords.dim() != 2 or not 1 <= coords.shape[1] <= _lib.MAX_DIM:
        raise NotImplementedError(f"loglik_svc serves 1 .. {_lib.MAX_DIM} coordinate columns")
    if nbr.dim() != 2 or not 1 <= nbr.shape[1] <= _lib.GRAD_MAX_M:
        raise NotImplementedError(f"loglik_svc's gradient serves 1 <= m <= {_lib.GRAD_MAX_M}")
    if nbr.shape[0] != coords.shape[0]:
        raise ValueError("loglik_svc is an S = T sweep: one nbr row per location")
    ll, p = _LogLikSvc.apply(coords, Z, nbr, theta, values, kind, order)
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


class _LogLikLmc(torch.autograd.Function):
    """The multivariate (LMC) sweep (``torch.ops.nngp.bf_grad_mv``): A (q, q), phi (q,), tau2 (q,); with ``obs``
    (masks, rows_max, n_obs) the packed-row sweep ``torch.ops.nngp.bf_grad_mv_obs``."""

    @staticmethod
    def forward(ctx, coords, nbr, A, phi, tau2, Y, kind, order, obs=None):
        from . import load_ops

        load_ops()
        q = phi.shape[0]
        host = [[float(x) for x in t.detach().cpu().reshape(-1).tolist()] for t in (A, phi, tau2)]  # host synchronisation
        vals, n_obs = Y.detach().reshape(-1, q, 1).contiguous(), nbr.shape[0] * q
        if obs is None:
            p, g, _ = torch.ops.nngp.bf_grad_mv(coords, nbr, order, 0, _lib.KIND_CODES[kind], *host, vals, False)
        else:
            masks, rows_max, n_obs = obs
            p, g, _ = torch.ops.nngp.bf_grad_mv_obs(coords, nbr, order, 0, _lib.KIND_CODES[kind], *host, vals, masks,
                                                    rows_max, False)
        ctx.save_for_backward(g)
        ctx.meta = (q, A.device, phi.device, tau2.device)
        ctx.mark_non_differentiable(p)
        ll = -0.5 * (n_obs * math.log(2.0 * math.pi) + p[0] + p[1])
        return ll, p

    @staticmethod
    def backward(ctx, grad_out, _grad_p):
        (g,) = ctx.saved_tensors
        q, adev, pdev, tdev = ctx.meta
        g = grad_out * g
        ntq = q * (q + 1) // 2
        gA = None
        if ctx.needs_input_grad[2]:
            low = torch.tril_indices(q, q, device=g.device)  # row-major: the order of the sweep's gradient
            gA = torch.zeros((q, q), dtype=g.dtype, device=g.device).index_put((low[0], low[1]), g[:ntq]).to(adev)
        gphi = g[ntq:ntq + q].to(pdev) if ctx.needs_input_grad[3] else None
        gtau = g[ntq + q:].to(tdev) if ctx.needs_input_grad[4] else None
        return None, None, gA, gphi, gtau, None, None, None, None


def loglik_lmc(coords, nbr, kind, A, phi, tau2, Y, order=None):
    """NNGP log-likelihood of ``Y`` (N, q) on S = T under the linear model of coregionalisation
    (:class:`LMCCovariance`): ``A`` (q, q) lower-triangular, ``phi`` (q,) and ``tau2`` (q,) float64 tensors,
    differentiable in all three (zeros above A's diagonal get zero gradient).

    Forward runs one gradient sweep (``torch.ops.nngp.bf_grad_mv``) and synchronises with the host as :func:`loglik`
    does; backward returns ``grad_out * grad`` with no further launch.  ``nbr`` (N, m) int32, 2 <= q <= 4,
    (m + 1) q <= 64; kinds exponential, matern32, matern52, gaussian; the not-PD and bad-index flags raise.

    NaN in ``Y`` means "not observed": the packed-row gradient sweep (``torch.ops.nngp.bf_grad_mv_obs``) runs instead,
    over the observed entries only, with 1 <= m <= 63 and at most 64 observed neighbour rows per location (more is a
    ``ValueError`` before any launch).
    """
    if kind not in _lib.KIND_CODES:
        raise ValueError(f"unknown covariance kind {kind!r}")
    if any(t.dtype != torch.float64 for t in (A, phi, tau2)) or A.dim() != 2 or phi.dim() != 1 or \
            A.shape != (phi.shape[0],) * 2 or tau2.shape != phi.shape:
        raise ValueError("A must be a float64 (q, q) tensor, phi and tau2 float64 (q,)")
    if nbr.dim() != 2:
        raise ValueError("nbr must be int32 (N, m)")
    if nbr.shape[0] != coords.shape[0] or Y.shape != (coords.shape[0], phi.shape[0]):
        raise ValueError("loglik_lmc is an S = T sweep: one nbr row and one row of Y (N, q) per location")
    host = [t.detach().cpu().tolist() for t in (A, phi, tau2)]
    seen = ~torch.isnan(Y)
    obs = None
    if not bool(seen.all()):
        # bit a of a site's mask: outcome a observed; the bound on the packed rows before any launch
        masks = (seen.to(torch.int32) << torch.arange(phi.shape[0], dtype=torch.int32, device=Y.device)).sum(1)
        masks = masks.to(torch.uint8)
        rows = _lib.mv_obs_rows(nbr, masks)
        rows_max = int(rows.max()) if rows.numel() else 0
        if rows_max > _lib.MV_MAX_ROWS:
            raise ValueError(f"location {int(rows.argmax())} conditions on {rows_max} observed neighbour rows; the "
                             f"packed-row sweep serves at most {_lib.MV_MAX_ROWS}: use a smaller m")
        obs = (masks, max(rows_max, 1), int(seen.sum()))
        _lib._mv_obs_checks(kind, nbr.shape[1], *host, masks, coords.shape[0], obs[1])
    else:
        _lib._mv_checks(kind, nbr.shape[1], *host)
    _lib._require_gpu(coords, nbr, Y, order)
    ll, p = _LogLikLmc.apply(coords, nbr, A, phi, tau2, Y, kind, order, obs)
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
