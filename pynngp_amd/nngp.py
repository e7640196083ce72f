"""Drop-in ``NNGP`` class (mirrors ``pyNNGP.NNGP``, /root/reference/pyNNGP/nngp.py).

Same constructor ``NNGP(t, y, eps, refType, m, cov)`` (nngp.py:6-18), same
attributes ``t, y, eps, refType, m, cov, s, wt, ws, Ns, Nt`` and the same
per-location methods ``_Bsi, _CNs, _Ccross, _Fsi, _Cs`` (nngp.py:73-96) -- but the
neighbour sets, the B/F algebra and the log-likelihood run on the MI355X through
``libnngp_hip.so``.  Additions: the device-resident ``nbr`` / ``B`` / ``F`` arrays
and ``loglik()``, the sweep the reference's ``oneSample`` (nngp.py:98-101) needs.

Differences from the reference, all deliberate:
* ``cov`` is a :class:`Covariance` (kind + theta: the covariance fused into the kernel, the
  fast path), an :class:`IsotropicCovariance` (a torch function of distance), or -- as in the
  reference -- any Python callable ``cov(a, b)`` on coordinate rows (the reference passes index
  arrays at nngp.py:82, a bug; here the rows).  A callable drives ``_CNs/_Ccross/_Cs`` directly
  and ``_Bsi/_Fsi/compute_BF/loglik/predict`` through :class:`CallableCovariance` (its joint
  blocks evaluated, then factorised on the GPU by the covariance-block kernels, 1 <= m <= 32).
  ``cov=None`` (the reference test) builds neighbour sets only.
* exact distance ties are ordered by lower index (the reference's is arbitrary).
* tuple ``refType`` values work as the reference's comments describe
  (nngp.py:23-27, with the same ``np.random`` calls as nngp.py:36-40, so a seeded
  global RNG gives the S the reference meant to draw); the reference itself raises
  ``AttributeError`` there (``self.typ``, nngp.py:34).  An unknown string raises
  ``ValueError`` (the reference silently leaves ``s`` unset, nngp.py:29-31).
* ``Nt`` for refType != 'S=T' is a list of int64 index arrays into ``s`` (the
  reference appends ``(dist, ind)`` tuples, nngp.py:71, because ``return_distance``
  defaults to True); ``predict()`` evaluates B_t, F_t and the kriging mean at t
  (nngp_bf_cross).
"""
from __future__ import annotations

import dataclasses
import math
from typing import Callable, Optional, Union

import numpy as np
import torch

from . import _lib

LOG_2PI = math.log(2.0 * math.pi)


@dataclasses.dataclass(frozen=True)
class Covariance:
    """Parent-GP covariance plug-in (the reference's ``cov``, nngp.py:6,12), u = phi d:

    ``exponential`` sigma2 e^-u; ``matern32`` sigma2 (1 + u) e^-u; ``matern52``
    sigma2 (1 + u + u^2/3) e^-u; ``gaussian`` sigma2 e^-u^2; ``spherical``
    sigma2 (1 - 3u/2 + u^3/2) for u < 1, else 0 (the spNNGP family, fused in the kernels);
    ``matern`` sigma2 u^nu K_nu(u) / (2^(nu-1) Gamma(nu)) for any smoothness ``nu`` in (0, 50]
    (spNNGP's "matern"; served by the wavefront kernel, nngp.h NNGP_COV_MATERN).
    ``tau2`` is a nugget added to the diagonal (response model; 0 = latent model).
    Called as ``cov(a, b)`` on coordinate rows of any dimension (numpy or torch), it
    returns the cross-covariance matrix without the nugget, like a reference plug-in would.
    """

    kind: str
    sigma2: float
    phi: float
    tau2: float = 0.0
    nu: Optional[float] = None  # smoothness of the ``matern`` kind (None for the others)

    def __post_init__(self):
        if self.kind not in _lib.KIND_CODES:
            raise ValueError(f"unknown covariance kind {self.kind!r}; expected one of {sorted(_lib.KIND_CODES)}")
        if not (self.sigma2 > 0 and self.phi > 0 and self.tau2 >= 0):
            raise ValueError("need sigma2 > 0, phi > 0, tau2 >= 0")
        _lib._check_kind(self.kind, self.nu)

    @property
    def nu_arg(self) -> Optional[float]:
        """``nu`` as the sweeps take it (None unless the kind is ``matern``)."""
        return float(self.nu) if self.kind == "matern" else None

    @property
    def theta(self):
        return (float(self.sigma2), float(self.phi), float(self.tau2))

    def replace(self, **kw) -> "Covariance":
        return dataclasses.replace(self, **kw)

    def __call__(self, a, b):
        lib = torch if isinstance(a, torch.Tensor) else np
        d = a.shape[-1] if a.ndim > 1 else b.shape[-1] if b.ndim > 1 else 1
        a = a.reshape(-1, d)
        b = b.reshape(-1, d)
        t = a[:, None, :] - b[None, :, :]
        u = self.phi * lib.sqrt((t * t).sum(-1))
        if self.kind == "matern":  # K_nu of real order: scipy on the host (torch has only K_0, K_1)
            from scipy import special
            un = u.detach().cpu().numpy() if lib is torch else u
            us = np.where(un > 0, un, 1.0)
            with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
                k = special.kv(self.nu, us)
                r = np.exp(self.nu * np.log(us) - (self.nu - 1.0) * np.log(2.0) - special.gammaln(self.nu) + np.log(k))
            r = self.sigma2 * np.where((un > 0) & np.isfinite(k), r, 1.0)
            return torch.as_tensor(r, dtype=u.dtype, device=u.device) if lib is torch else r
        if self.kind == "gaussian":
            return self.sigma2 * lib.exp(-u * u)
        if self.kind == "spherical":
            return lib.where(u < 1.0, self.sigma2 * (1.0 - 1.5 * u + 0.5 * u * u * u), 0.0 * u)
        e = self.sigma2 * lib.exp(-u)
        if self.kind == "matern32":
            return e * (1.0 + u)
        if self.kind == "matern52":
            return e * (1.0 + u + u * u / 3.0)
        return e


@dataclasses.dataclass(frozen=True, init=False)
class MaternCovariance(Covariance):
    """The general-smoothness Matern covariance with the smoothness as a fourth parameter:
    ``MaternCovariance(sigma2, phi, tau2, nu)``, ``theta`` = (sigma2, phi, tau2, nu).

    Forward it is ``Covariance("matern", sigma2, phi, tau2, nu=nu)`` -- the same sweeps, the same bits.  It is the
    type by which :meth:`NNGP.loglik_grad`, :meth:`NNGP.profile_loglik_grad` and ``fit(estimate_nu=...)`` select the
    four-component gradient sweep (``nngp_bf_grad_matern``), which ``Covariance("matern", ...)`` keeps refusing.
    The Fisher, latent-gradient and per-axis paths refuse it as they refuse the kind."""

    def __init__(self, sigma2: float, phi: float, tau2: float = 0.0, nu: Optional[float] = None):
        for k, v in (("kind", "matern"), ("sigma2", sigma2), ("phi", phi), ("tau2", tau2), ("nu", nu)):
            object.__setattr__(self, k, v)
        self.__post_init__()

    @property
    def theta(self):
        return (float(self.sigma2), float(self.phi), float(self.tau2), float(self.nu))

    def replace(self, **kw) -> "MaternCovariance":
        if kw.get("kind", "matern") != "matern":
            raise ValueError("a MaternCovariance is of kind 'matern'")
        f = {"sigma2": self.sigma2, "phi": self.phi, "tau2": self.tau2, "nu": self.nu}
        f.update({k: v for k, v in kw.items() if k != "kind"})
        return MaternCovariance(**f)


_ANISO_KINDS = ("exponential", "matern32", "matern52", "gaussian", "spherical")


@dataclasses.dataclass(frozen=True)
class AnisotropicCovariance:
    """A fused kind of :class:`Covariance` with one decay per axis: u = sqrt(sum_k (phi_k (a_k - b_k))^2)
    (geometric anisotropy along the axes; space x time, covariates as extra coordinates).  ``phi`` has one positive
    entry per coordinate column; kinds ``exponential`` .. ``spherical``.  The model equals the isotropic one at
    phi = 1 on the coordinates scaled column by column (:meth:`scaled`), which is how the forward sweeps run it;
    the gradient in (sigma2, phi_1 .. phi_dim, tau2) comes from ``nngp_bf_grad_aniso``.  Called as ``cov(a, b)`` on
    coordinate rows it returns the cross-covariance matrix without the nugget."""

    kind: str
    sigma2: float
    phi: tuple
    tau2: float = 0.0

    def __post_init__(self):
        if self.kind not in _ANISO_KINDS:
            raise ValueError(f"AnisotropicCovariance serves the kinds {_ANISO_KINDS}, got {self.kind!r}")
        try:
            phi = tuple(float(p) for p in self.phi)
        except TypeError:
            raise ValueError("phi must be a sequence with one decay per coordinate axis") from None
        if not 1 <= len(phi) <= _lib.MAX_DIM:
            raise ValueError(f"phi must have 1 .. {_lib.MAX_DIM} entries (one per coordinate axis), got {len(phi)}")
        if not all(p > 0 and math.isfinite(p) for p in phi):
            raise ValueError(f"every phi_k must be positive and finite, got {phi}")
        if not (self.sigma2 > 0 and math.isfinite(self.sigma2) and self.tau2 >= 0 and math.isfinite(self.tau2)):
            raise ValueError("need sigma2 > 0, tau2 >= 0 (finite)")
        object.__setattr__(self, "phi", phi)

    nu = None
    nu_arg = None

    @property
    def dim(self) -> int:
        return len(self.phi)

    @property
    def theta(self):
        return (float(self.sigma2), *self.phi, float(self.tau2))

    def replace(self, **kw) -> "AnisotropicCovariance":
        return dataclasses.replace(self, **kw)

    def scaled(self):
        """``(Covariance(kind, sigma2, 1.0, tau2), phi_vec)``: the isotropic covariance on ``coords * phi_vec``."""
        return Covariance(self.kind, self.sigma2, 1.0, self.tau2), np.array(self.phi, dtype=np.float64)

    def __call__(self, a, b):
        lib = torch if isinstance(a, torch.Tensor) else np
        d = self.dim
        if (a.ndim > 1 and a.shape[-1] != d) or (b.ndim > 1 and b.shape[-1] != d):
            raise ValueError(f"coordinate rows must have {d} columns (len(phi))")
        s = torch.tensor(self.phi, dtype=a.dtype, device=a.device) if lib is torch else np.array(self.phi)
        return self.scaled()[0](a.reshape(-1, d) * s, b.reshape(-1, d) * s)


_SEP_KINDS = _ANISO_KINDS


@dataclasses.dataclass(frozen=True)
class SeparableCovariance:
    """The separable space-time product ``sigma2 rho_s(phi_s |a_s - b_s|) rho_t(phi_t |a_t - b_t|) + tau2 delta_ab``:
    the last coordinate column is time, the first dim - 1 columns (dim 2 or 3) are space.  ``kind_s`` and ``kind_t``
    name the two correlations, ``exponential`` .. ``spherical`` each.  The sweeps evaluate it fused
    (``nngp_bf_sweep_sep``, ``nngp_bf_cross_sep``, ``nngp_bf_grad_sep``); the gradient is in
    (sigma2, phi_s, phi_t, tau2).  An :class:`AnisotropicCovariance` is the *metric* model
    rho(sqrt(phi_s^2 d_s^2 + phi_t^2 d_t^2)) instead; the two agree only for gaussian x gaussian.  Called as
    ``cov(a, b)`` on coordinate rows it returns the cross-covariance matrix without the nugget.

    Neighbour sets come from the ordinary search on the coordinates scaled column by column by :meth:`scaled`
    (phi_s, .., phi_s, phi_t).  For a product correlation that is a heuristic: the scaled Euclidean distance does not
    order pairs by their correlation (it does for gaussian x gaussian only)."""

    kind_s: str
    kind_t: str
    sigma2: float
    phi_s: float
    phi_t: float
    tau2: float = 0.0

    def __post_init__(self):
        for k in (self.kind_s, self.kind_t):
            if k not in _SEP_KINDS:
                raise ValueError(f"SeparableCovariance serves the kinds {_SEP_KINDS} for each factor, got {k!r}")
        th = (self.sigma2, self.phi_s, self.phi_t, self.tau2)
        if not all(isinstance(x, (int, float, np.floating, np.integer)) and math.isfinite(x) for x in th):
            raise ValueError(f"sigma2, phi_s, phi_t, tau2 must be finite numbers, got {th}")
        if not (self.sigma2 > 0 and self.phi_s > 0 and self.phi_t > 0 and self.tau2 >= 0):
            raise ValueError("need sigma2 > 0, phi_s > 0, phi_t > 0, tau2 >= 0")

    nu = None
    nu_arg = None

    @property
    def theta(self):
        return (float(self.sigma2), float(self.phi_s), float(self.phi_t), float(self.tau2))

    def replace(self, **kw) -> "SeparableCovariance":
        return dataclasses.replace(self, **kw)

    def scaled(self, dim: int = 3):
        """The per-column scales (phi_s, .., phi_s, phi_t) for ``dim`` coordinate columns: the metric of the
        neighbour search (a heuristic for a product correlation, see the class)."""
        if dim not in (2, 3):
            raise ValueError(f"SeparableCovariance serves 2 or 3 coordinate columns (space, then time), got {dim}")
        return np.array([self.phi_s] * (dim - 1) + [self.phi_t], dtype=np.float64)

    def __call__(self, a, b):
        d = a.shape[-1] if a.ndim > 1 else b.shape[-1]
        if d not in (2, 3) or (a.ndim > 1 and a.shape[-1] != d) or (b.ndim > 1 and b.shape[-1] != d):
            raise ValueError("coordinate rows must have 2 or 3 columns (space, then time)")
        a, b = a.reshape(-1, d), b.reshape(-1, d)
        cs = Covariance(self.kind_s, 1.0, self.phi_s, 0.0)(a[:, :d - 1], b[:, :d - 1])
        ct = Covariance(self.kind_t, 1.0, self.phi_t, 0.0)(a[:, d - 1:], b[:, d - 1:])
        return self.sigma2 * cs * ct


def _refuse_sep(cov, what: str) -> None:
    if isinstance(cov, SeparableCovariance):
        raise TypeError(f"{what} does not serve a SeparableCovariance (space x time product): use loglik / "
                        "compute_BF / predict(query=) / profile_loglik / profile_loglik_grad / gls / loglik_grad / fit "
                        "on refType='S=T'")


def _refuse_aniso(cov, what: str) -> None:
    _refuse_sep(cov, what)
    if isinstance(cov, AnisotropicCovariance):
        raise TypeError(f"{what} does not serve an AnisotropicCovariance (per-axis ranges): it would need the "
                        "range of every axis; use loglik / profile_loglik / loglik_grad / fit(anisotropic=True), or "
                        "a Covariance on coordinates you scaled yourself")


@dataclasses.dataclass(frozen=True)
class IsotropicCovariance:
    """A covariance of the caller's own -- the reference's `cov` plug-in (nngp.py:6,12) as any
    isotropic function of distance -- driving the fused GPU sweep: ``fn`` maps a float64 torch
    tensor of distances (any shape, on the GPU) to covariances elementwise (without the nugget;
    C(0) = ``fn(0)`` is the marginal variance), ``tau2`` is the nugget.  The sweep evaluates
    ``fn`` once over every joint block's distances (``_lib.joint_dist``, +inf for slots without
    a point, whose entries the kernel then ignores) and factorises the blocks in the
    ``bf_pairb`` kernel reading them from memory (nngp_bf_sweep_blocks, 1 <= m <= 24).
    Example: ``IsotropicCovariance(lambda d: 2.0 * torch.exp(-(d / 0.1) ** 1.5), tau2=0.1)``
    (a powered exponential).  Called as ``cov(a, b)`` on coordinate rows it returns the
    cross-covariance matrix, like a reference plug-in."""

    fn: Callable
    tau2: float = 0.0
    name: str = "custom"

    def __post_init__(self):
        if not callable(self.fn):
            raise TypeError("fn must be callable (a torch function of distance)")
        if not self.tau2 >= 0:
            raise ValueError("need tau2 >= 0")

    kind = "custom"

    @property
    def sigma2(self) -> float:
        """C(0) = fn(0), evaluated on the GPU when there is one (``fn`` may be a GPU-only function,
        e.g. one built on ``_lib.matern``)."""
        return self.variance("cuda" if torch.cuda.is_available() else "cpu")

    def variance(self, device) -> float:
        """C(0) = fn(0) evaluated on ``device``."""
        return float(self.fn(torch.zeros(1, dtype=torch.float64, device=device)).item())

    def marginal(self, points: torch.Tensor) -> torch.Tensor:
        """C(x, x) + tau2 at every point (the m = 0 prediction variance)."""
        return torch.full((points.shape[0],), self.variance(points.device) + self.tau2, dtype=torch.float64,
                          device=points.device)

    def blocks(self, dist: torch.Tensor, m: int) -> torch.Tensor:
        """Covariance blocks for :func:`_lib.bf_sweep_blocks`: fn over the distances, tau2 on the
        diagonal entries."""
        c = self.fn(dist)
        if not isinstance(c, torch.Tensor) or c.shape != dist.shape:
            raise ValueError("fn must return a tensor of the distances' shape")
        c = c.to(torch.float64).contiguous()
        if self.tau2 > 0:
            diag = _lib.joint_diagonal(m).to(c.device)
            c[diag] += self.tau2
        return c

    def __call__(self, a, b):
        to_np = not isinstance(a, torch.Tensor)
        ta = torch.as_tensor(np.asarray(a, dtype=np.float64)) if to_np else a
        tb = torch.as_tensor(np.asarray(b, dtype=np.float64)) if to_np else b
        d = ta.shape[-1] if ta.dim() > 1 else tb.shape[-1] if tb.dim() > 1 else 1
        ta, tb = ta.reshape(-1, d), tb.reshape(-1, d)
        t = ta[:, None, :] - tb[None, :, :]
        c = self.fn(torch.sqrt((t * t).sum(-1)))
        return c.cpu().numpy() if to_np else c


class CallableCovariance:
    """The reference's ``cov`` plug-in as it stands (``pyNNGP/nngp.py:6,12``): any callable
    ``fn(a, b)`` that maps two sets of coordinate rows (k_a, d) and (k_b, d) to their
    cross-covariance matrix (k_a, k_b) -- the call ``_CNs`` makes on the neighbours' rows
    (``nngp.py:82``) and ``_Cs`` on a location's row (``nngp.py:96``).  No isotropy or other
    structure is assumed (e.g. an anisotropic exponential exp(-sqrt((a-b)^T A (a-b)))).

    It drives the device sweep through the covariance-block kernels: for every location the joint
    block ``fn(X, X)`` of X = [its neighbours' rows; its own row] is evaluated, packed into
    ``_lib.bf_sweep_blocks``'s layout (lower triangle, entry-major) and factorised on the GPU
    (``nngp_bf_sweep_blocks``: B, F, residuals and the log-likelihood partials; 1 <= m <= 32).
    Evaluation, chosen once per object by probing ``fn`` on a few rows against one call per row:
      * ``"torch"``: ``fn`` broadcasts over a leading batch dimension of torch tensors on the GPU --
        one call per chunk of rows with X of shape (rows, m+1, d), on the device;
      * ``"numpy"``: the same with numpy arrays (host evaluation of the user's function, one call
        per chunk; the blocks then go to the GPU);
      * ``"loop"``: one call per location with the (m+1, d) numpy rows the reference passes.
    ``batch`` forces a mode.  The covariance values are the caller's code; everything after them
    (the factorisation, B, F, the log-likelihood) runs on the GPU, with no CPU path.
    ``tau2`` is an optional nugget added to the diagonal (0: ``fn``'s own values are C)."""

    kind = "custom"
    MODES = ("torch", "numpy", "loop", "loop_torch")

    def __init__(self, fn: Callable, tau2: float = 0.0, batch: Optional[str] = None, chunk_bytes: int = 1 << 28,
                 cache: bool = False, pairs: bool = False):
        if not callable(fn):
            raise TypeError("cov must be callable as cov(a, b) on coordinate rows")
        if not tau2 >= 0:
            raise ValueError("need tau2 >= 0")
        if batch is not None and batch not in self.MODES:
            raise ValueError(f"batch must be one of {self.MODES} or None")
        self.fn, self.tau2, self.batch, self.chunk_bytes = fn, float(tau2), batch, int(chunk_bytes)
        self.mode = batch
        # pairs=True: in "torch" mode, evaluate fn once per DISTINCT point pair of a sweep's joint blocks and
        # gather the blocks from those values (N = 1e6, m = 15: 30.5 M pairs instead of 136 M block entries),
        # when fn on single-row pairs reproduces its joint blocks bit for bit in both argument orders (probed
        # once).  Opt-in: the pair index costs ~42 ms per neighbour set (then cached), and a cheap broadcasting
        # plug-in evaluates (P, 1, 1)-shaped pairs at a lower per-element rate than whole blocks (17.2 against
        # 19.0 ms per sweep's blocks, profiles/r05o) -- it pays for an expensive fn reused over many sweeps
        self.pairs = pairs
        self._pairs_ok = None
        self._pidx = None  # (coords, nbr, order, i0, versions) -> the distinct pairs and the blocks' gather index
        # cache=True: NNGP keeps this covariance's evaluated joint blocks between sweeps (the caller promises
        # fn is a fixed function: no state it reads changes).  Default off, as the reference, which calls cov
        # on every evaluation (nngp.py:82,96): a mutable plug-in (an MLE loop over a closure's parameters)
        # then always sees its current state.
        self.cache = bool(cache)

    def __call__(self, a, b):
        return self.fn(a, b)

    # -- evaluation modes --------------------------------------------------------
    def _eval(self, X: torch.Tensor, mode: str) -> torch.Tensor:
        """fn's joint blocks (r, k, k) on X's device for X (r, k, d)."""
        if mode == "torch":
            C = self.fn(X, X)
            if not isinstance(C, torch.Tensor):
                raise TypeError("not a torch tensor")
            return C.to(device=X.device, dtype=torch.float64)
        Xh = X.detach().cpu().numpy()
        if mode == "numpy":
            C = np.asarray(self.fn(Xh, Xh), dtype=np.float64)
        elif mode == "loop":
            C = np.stack([np.asarray(self.fn(x, x), dtype=np.float64).reshape(x.shape[0], x.shape[0]) for x in Xh]) \
                if Xh.shape[0] else np.zeros((0, X.shape[1], X.shape[1]))
        else:  # loop_torch: one call per location with torch rows on the device
            return torch.stack([torch.as_tensor(self.fn(x, x), dtype=torch.float64, device=X.device).reshape(
                x.shape[0], x.shape[0]) for x in X]) if X.shape[0] else X.new_zeros((0, X.shape[1], X.shape[1]))
        return torch.from_numpy(np.ascontiguousarray(C)).to(X.device)

    def resolve_mode(self, X: torch.Tensor) -> str:
        """Pick (once) the fastest evaluation that reproduces one call per location on sample rows X
        (r, k, d): relative 1e-13 (a batched expression may round in a different order)."""
        if self.mode is not None:
            return self.mode
        ref, ref_mode = None, None
        for lm in ("loop", "loop_torch"):
            try:
                ref = self._eval(X, lm).cpu().numpy()
                ref_mode = lm
                break
            except Exception:  # noqa: BLE001 -- the plug-in decides what it accepts
                continue
        if ref is None:
            raise TypeError("cov(a, b) failed on the joint blocks' coordinate rows (numpy and torch (k, d) inputs)")
        k = X.shape[1]
        if ref.shape != (X.shape[0], k, k) or not np.all(np.isfinite(ref)):
            raise ValueError(f"cov(a, b) must return a finite ({k}, {k}) matrix for two ({k}, d) row sets")
        scale = float(np.max(np.abs(ref))) if ref.size else 1.0
        for bm in ("torch", "numpy"):
            try:
                C = self._eval(X, bm)
            except Exception:  # noqa: BLE001
                continue
            if tuple(C.shape) == ref.shape and np.allclose(C.cpu().numpy(), ref, rtol=1e-13, atol=1e-15 * scale):
                self.mode = bm
                return bm
        self.mode = ref_mode
        return ref_mode

    def _pairs_probe(self, X: torch.Tensor, ta: torch.Tensor, tb: torch.Tensor) -> bool:
        """fn on (P, 1, d) single-row pairs equals its joint blocks' entries bit for bit, in both argument
        orders (the distinct pairs are keyed by (smaller, larger) point index)."""
        if self._pairs_ok is None:
            try:
                C = self._eval(X, "torch")[:, ta, tb].reshape(-1)
                xa, xb = X[:, ta].reshape(-1, 1, X.shape[2]), X[:, tb].reshape(-1, 1, X.shape[2])
                ab = torch.as_tensor(self.fn(xa, xb), dtype=torch.float64, device=X.device).reshape(-1)
                ba = torch.as_tensor(self.fn(xb, xa), dtype=torch.float64, device=X.device).reshape(-1)
                self._pairs_ok = bool(torch.equal(ab, C) and torch.equal(ba, C))
            except Exception:  # noqa: BLE001 -- the plug-in decides what it accepts
                self._pairs_ok = False
        return self._pairs_ok

    def _pair_index(self, coords, nbr, i0, order, ta, tb):
        """The sweep's distinct point pairs (pa, pb: point indices, pa <= pb) and the blocks' gather index
        inv ((m+1)(m+2)/2, rows) into [0, values...] (0: an entry with a slot without a point -- unused by
        the kernels); cached for the same coords / nbr / order tensors (held, and their versions checked)."""
        key = (coords, nbr, order, int(i0), coords._version, nbr._version, None if order is None else order._version)
        c = self._pidx
        if c is not None and all(x is y for x, y in zip(c[0][:3], key[:3])) and c[0][3:] == key[3:]:
            return c[1]
        n = coords.shape[0]
        rows = nbr.shape[0]
        loc = (torch.arange(rows, device=nbr.device) if order is None else order.long()) + int(i0)
        idx = nbr.long()
        g = torch.cat([torch.where((idx >= 0) & (idx < n), idx, torch.full_like(idx, -1)), loc[:, None]], dim=1)
        ga, gb = g[:, ta].t(), g[:, tb].t()  # entry-major (ne, rows)
        keys = torch.where((ga >= 0) & (gb >= 0), torch.minimum(ga, gb) * n + torch.maximum(ga, gb),
                           torch.full_like(ga, -1))
        del g, ga, gb
        uniq, inv = torch.unique(keys, return_inverse=True)
        del keys
        # slot 0 of the values is the unused entries' (a key of -1 sorts first when present)
        if uniq.numel() and int(uniq[0]) < 0:
            uniq = uniq[1:]
        else:
            inv += 1
        res = (uniq // n, uniq % n, inv)
        self._pidx = (key, res)
        return res

    def blocks(self, coords: torch.Tensor, nbr: torch.Tensor, i0: int = 0, qcoords: Optional[torch.Tensor] = None,
               order: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Joint blocks in :func:`_lib.bf_sweep_blocks`'s layout ((m+1)(m+2)/2, rows): fn over
        [neighbour rows; the location's row] for every nbr row (a slot without a point repeats the
        location's row -- the kernel ignores its entries), tau2 on the diagonal entries."""
        m = nbr.shape[1]
        rows = nbr.shape[0]
        dev = nbr.device
        ne = (m + 1) * (m + 2) // 2
        out = torch.empty((ne, rows), dtype=torch.float64, device=dev)
        if rows == 0:
            return out
        a = torch.arange(m + 1, device=dev)
        ta = torch.repeat_interleave(a, a + 1)  # entry e = a (a+1)/2 + b: rows a, then b = 0..a
        tb = torch.cat([torch.arange(int(k) + 1, device=dev) for k in range(m + 1)])
        per_row = (m + 1) * (m + 1) * 8 * 3 + (m + 1) * coords.shape[1] * 8
        chunk = max(1, min(rows, self.chunk_bytes // per_row))
        X4 = joint_points(coords, nbr[:min(rows, 4)], i0, qcoords, None if order is None else order[:min(rows, 4)])
        mode = self.resolve_mode(X4)
        if (self.pairs and mode == "torch" and qcoords is None and dev.type == "cuda" and rows * ne < 2 ** 31
                and coords.shape[0] < 2 ** 31 and self._pairs_probe(X4, ta, tb)):
            pa, pb, inv = self._pair_index(coords, nbr, i0, order, ta, tb)
            vals = torch.empty(pa.numel() + 1, dtype=torch.float64, device=dev)
            vals[0] = 0.0
            # (a pair is a few doubles of fn's temporaries: chunks of millions of pairs keep the launches few)
            pchunk = max(1, 8 * self.chunk_bytes // (8 * (3 + 2 * coords.shape[1])))
            for p0 in range(0, pa.numel(), pchunk):
                p1 = min(pa.numel(), p0 + pchunk)
                C = self.fn(coords[pa[p0:p1]][:, None, :], coords[pb[p0:p1]][:, None, :])
                vals[1 + p0:1 + p1] = torch.as_tensor(C, dtype=torch.float64, device=dev).reshape(-1)
            torch.index_select(vals, 0, inv.reshape(-1), out=out.view(-1))
            if self.tau2 > 0:
                out[_lib.joint_diagonal(m).to(dev)] += self.tau2
            return out
        if mode.startswith("loop"):
            chunk = min(chunk, 4096)
        for r0 in range(0, rows, chunk):
            r1 = min(rows, r0 + chunk)
            # (rows r0.. of a sweep without a visiting order are the locations i0 + r0 ..: round 5 fix -- the
            # chunks after the first took i0 .. again, wrong blocks once rows exceeded one chunk, e.g. m = 27
            # beyond ~14 k rows; found by the distinct-pair evaluation's bit-identity test)
            X = joint_points(coords, nbr[r0:r1], i0 + (r0 if order is None else 0), qcoords,
                             None if order is None else order[r0:r1])
            C = self._eval(X, mode)
            if tuple(C.shape) != (r1 - r0, m + 1, m + 1):
                raise ValueError(f"cov(a, b) returned {tuple(C.shape)} for {r1 - r0} joint blocks of {m + 1} rows")
            out[:, r0:r1] = C[:, ta, tb].t()
        if self.tau2 > 0:
            out[_lib.joint_diagonal(m).to(dev)] += self.tau2
        return out

    def marginal(self, points: torch.Tensor) -> torch.Tensor:
        """C(x, x) + tau2 at every point (the m = 0 prediction variance): fn on each row alone."""
        X = points[:, None, :]
        return self._eval(X, self.resolve_mode(X[:4]))[:, 0, 0] + self.tau2


def joint_points(coords: torch.Tensor, nbr: torch.Tensor, i0: int = 0, qcoords: Optional[torch.Tensor] = None,
                 order: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Coordinates of every joint block, (rows, m+1, d): slots 0..m-1 the neighbours ``coords[nbr]``
    (a slot without a point -- index -1 or out of range -- repeats the location's row), slot m the
    location ``qcoords[i0 + (order[t] if order else t)]`` (``qcoords`` defaults to ``coords``)."""
    q = coords if qcoords is None else qcoords
    rows = nbr.shape[0]
    loc = (torch.arange(rows, device=nbr.device) if order is None else order.long()) + int(i0)
    xi = q[loc]
    idx = nbr.long()
    ok = (idx >= 0) & (idx < coords.shape[0])
    xn = coords[torch.where(ok, idx, torch.zeros_like(idx))]
    xn = torch.where(ok[..., None], xn, xi[:, None, :])
    return torch.cat([xn, xi[:, None, :]], dim=1)


CovLike = Union[Covariance, AnisotropicCovariance, IsotropicCovariance, CallableCovariance, Callable, None]


def _sweep_any(cv, coords, nbr, i0=0, values=None, want_bf=True, algo="auto", order=None, R=None, qcoords=None,
               qvalues=None, blocks=None):
    """One fused sweep for any covariance form: a built-in kind (nngp_bf_sweep / nngp_bf_cross),
    an :class:`IsotropicCovariance` (joint distances -> fn -> nngp_bf_sweep_blocks) or a
    :class:`CallableCovariance` (fn(a, b) on the joint blocks' rows -> nngp_bf_sweep_blocks;
    ``blocks``: already evaluated blocks of these rows, e.g. cached).  ``qcoords``
    given: the cross sweep of those query points against ``coords`` (prediction); ``qvalues``: the
    values at the locations (S = T sweep: pass ``values``).  A :class:`SeparableCovariance` runs on its own fused
    sweeps (nngp_bf_sweep_sep / nngp_bf_cross_sep; ``algo`` is not used)."""
    if isinstance(cv, SeparableCovariance):
        want_r = R is not None
        if qcoords is not None:
            B, F, Rn, p = _lib.bf_cross_sep(coords, qcoords, nbr, cv.kind_s, cv.kind_t, *cv.theta, ref_values=values,
                                            query_values=qvalues, q0=i0, order=order, want_r=want_r)
        else:
            B, F, Rn, p = _lib.bf_sweep_sep(coords, nbr, i0, cv.kind_s, cv.kind_t, *cv.theta, values=values,
                                            want_bf=want_bf, order=order, want_r=want_r)
        if want_r:
            R.copy_(Rn)
        return B, F, p
    if isinstance(cv, (IsotropicCovariance, CallableCovariance)):
        m = nbr.shape[1]
        if not 1 <= m <= _lib.BLOCKS_MAX_M:
            raise ValueError(f"a custom covariance needs 1 <= m <= {_lib.BLOCKS_MAX_M} (the covariance-block kernels)")
        if algo not in ("auto", "pairb", "quad"):
            raise ValueError(f"a custom covariance runs on the covariance-block kernels, not algo {algo!r}")
        if blocks is None and isinstance(cv, CallableCovariance):
            blocks = cv.blocks(coords, nbr, i0, qcoords=qcoords, order=order)
        elif blocks is None:
            dist = _lib.joint_dist(coords, nbr, i0, qcoords=qcoords, order=order)
            blocks = cv.blocks(dist, m)
            del dist
        nq = (coords if qcoords is None else qcoords).shape[0]
        return _lib.bf_sweep_blocks(blocks, nbr, coords.shape[0], i0, values=values, qvalues=qvalues, want_bf=want_bf,
                                    order=order, R=R, n_locs=nq)
    if qcoords is not None:
        return _lib.bf_cross(coords, qcoords, nbr, cv.kind, *cv.theta[:3], ref_values=values, query_values=qvalues,
                             q0=i0, algo=algo, R=R, nu=cv.nu_arg)
    return _lib.bf_sweep(coords, nbr, i0, cv.kind, *cv.theta[:3], values=values, want_bf=want_bf, algo=algo, order=order,
                         R=R, nu=cv.nu_arg)


_NOISE_SCOPE = ("per-point noise (noise=) serves refType='S=T', a Covariance of kind exponential .. spherical, "
                "1 <= m <= 32 and mean='constant' or 'zero'")


def _refuse_noise(what: str):
    raise NotImplementedError(f"{what} is not served with noise=: {_NOISE_SCOPE}")


class _NoiseVar:
    """Validated per-point noise weights v = e^2 on the device (what ``noise=`` resolves to; a fit resolves once)."""

    def __init__(self, v: torch.Tensor):
        self.v = v


def _default_device(device):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise _lib.NNGPExtensionError("pynngp_amd.NNGP needs a ROCm GPU (torch.cuda.is_available() is False)")
    return torch.device("cuda", torch.cuda.current_device())


class NNGP:
    """Nearest-neighbour GP over ordinates ``t`` (mirrors ``pyNNGP.NNGP``).

    The model order.  Every reference point conditions on its ``m`` nearest *earlier* reference points, so the
    order of the reference set is part of the model.  ``ordering=None`` (the default) takes the caller's row
    order, as the reference does.  ``ordering="maxmin"`` (the levelled max-min order, :mod:`pynngp_amd.ordering`),
    ``"random"`` or an explicit permutation orders the reference set before the neighbour sets are built:

    * ``refType='S=T'``: ``t``, ``y`` and a per-point ``eps`` are permuted together, and the instance then lives
      entirely in model order -- its attributes ``t, y, eps, s, ws, wt``, every ``values=`` / ``X=`` argument,
      ``nbr``, ``B``, ``F`` and every per-location result are in model order.  ``model.perm`` (device int64,
      ``perm[k]`` = the input row at model position ``k``; ``None`` without an ordering) and
      ``model.to_model_order(a)`` / ``model.to_input_order(a)`` (rows of a numpy array or a tensor) convert
      between the two.
    * a tuple ``refType``: only the reference set ``s`` is ordered (``perm`` then indexes the drawn ``s``);
      ``t`` and ``y`` keep the caller's order.

    ``refType=("maxmin", nRef)`` takes as ``s`` the first ``nRef`` points of the max-min order of ``t``, in that
    order: distinct, space-filling points (``('subset', nRef)`` draws with replacement).
    """

    def __new__(cls, t=None, *args, **kw):
        # ordinates of 4 .. 16 columns run on a second, self-contained path (pynngp_amd.nd.NNGPnd, a subclass whose
        # own __init__ Python then calls); everything else is this class as before
        if cls is NNGP:
            from . import nd

            if nd.is_nd_points(t) and np.shape(t)[1] <= _lib.ND_MAX_DIM:
                return object.__new__(nd.NNGPnd)
        return object.__new__(cls)

    def __init__(self, t, y, eps, refType, m, cov: CovLike, device=None, ordering=None):
        self.t = t  # ordinates (held by reference, nngp.py:7)
        self.y = y  # abscissae
        # measurement uncertainties in y (nngp.py:9): per-point noise sigmas for oneSample, latent_posterior and,
        # through noise="eps", the response model (loglik, loglik_grad, profile_loglik, fit, predict)
        self.eps = eps
        self.refType = refType
        self.m = int(m)
        self.cov = cov
        self.device = _default_device(device)
        if not 0 <= self.m <= _lib.MAX_M:
            raise ValueError(f"m={m} outside [0, {_lib.MAX_M}]")
        self.perm = None
        self._ordering = ordering
        if ordering is not None and self._same_sets():
            self._order_inputs(ordering)

        self._init_s()
        # the metric of the neighbour search: the per-axis decays of an AnisotropicCovariance, else the plain one
        self._nbr_phi = self._metric_phi(cov)
        self._init_wt()
        self._init_ws()
        self._make_s_neighbor_sets()
        self._make_t_neighbor_sets()
        self._B = self._F = None

    # -- the model order ---------------------------------------------------------
    def _host_points(self, a, what: str) -> np.ndarray:
        """``a`` as finite float64 (n, d) host points, d <= 3 (what an ordering is computed from)."""
        p = np.ascontiguousarray(a, dtype=np.float64)
        if p.ndim == 1:
            p = p[:, None]
        if p.ndim != 2 or not 1 <= p.shape[1] <= _lib.MAX_DIM:
            raise ValueError(f"{what} must be (N, d) with 1 <= d <= {_lib.MAX_DIM}, got {tuple(p.shape)}")
        if not np.all(np.isfinite(p)):
            raise ValueError(f"Input contains NaN or infinity ({what})")
        return p

    def _order_inputs(self, ordering):
        """'S=T' with an ordering: permute t, y and a per-point eps together; the instance is in model order."""
        from . import ordering as _ordering

        t_host = self._host_points(self.t, "ordinates t")
        n = t_host.shape[0]
        perm = _ordering.resolve(ordering, torch.as_tensor(t_host).to(self.device))
        self.perm = torch.as_tensor(perm).to(self.device)
        self.t = np.asarray(self.t)[perm]
        y = np.asarray(self.y)
        if y.shape[:1] != (n,):
            raise ValueError(f"y must have one row per ordinate ({n}), got {tuple(y.shape)}")
        self.y = y[perm]
        if self.eps is not None and np.ndim(self.eps) >= 1 and np.shape(self.eps)[0] == n:
            self.eps = np.asarray(self.eps)[perm]

    def _order_reference(self, ordering):
        """A tuple refType with an ordering: the drawn reference set alone is put into model order."""
        from . import ordering as _ordering

        s_host = self._host_points(self.s, "reference set s")
        perm = _ordering.resolve(ordering, torch.as_tensor(s_host).to(self.device))
        self.perm = torch.as_tensor(perm).to(self.device)
        self.s = np.asarray(self.s)[perm]

    def to_model_order(self, a):
        """Rows of ``a`` (numpy array or tensor, one row per point of the ordered set, input order) in model
        order: ``a[perm]``.  Without an ordering: ``a`` itself."""
        perm = getattr(self, "perm", None)
        if perm is None:
            return a
        if torch.is_tensor(a):
            return a[perm.to(a.device)]
        return np.asarray(a)[perm.cpu().numpy()]

    def to_input_order(self, a):
        """The inverse of :meth:`to_model_order`: rows of a model-order ``a`` back at their input rows."""
        perm = getattr(self, "perm", None)
        if perm is None:
            return a
        if torch.is_tensor(a):
            out = torch.empty_like(a)
            out[perm.to(a.device)] = a
            return out
        a = np.asarray(a)
        out = np.empty_like(a)
        out[perm.cpu().numpy()] = a
        return out

    # -- construction (nngp.py:21-71) -----------------------------------------
    def _init_s(self):
        """Reference set S (nngp.py:21-40): 'S=T', ('subset', nRef), ('random', nRef, bounds) or
        ('maxmin', nRef)."""
        self.s = reference_set(self.t, self.refType, device=self.device)
        if getattr(self, "_ordering", None) is not None and self.s is not self.t:
            self._order_reference(self._ordering)
        t_host = np.ascontiguousarray(self.t, dtype=np.float64)
        if not np.all(np.isfinite(t_host)):  # as sklearn's KDTree / KNeighborsRegressor (nngp.py:46,55)
            raise ValueError("Input contains NaN or infinity (ordinates t)")
        if t_host.ndim == 1:  # a 1-D series given as a vector
            t_host = t_host[:, None]
        self._t_dev = torch.as_tensor(t_host).to(self.device)
        if self._t_dev.dim() != 2 or not 1 <= self._t_dev.shape[1] <= _lib.MAX_DIM:
            raise ValueError(f"ordinates must be (N, d) with 1 <= d <= {_lib.MAX_DIM}, got {tuple(self._t_dev.shape)}")
        if self.s is self.t:
            self._s_dev = self._t_dev
        else:
            s_host = np.ascontiguousarray(self.s, dtype=np.float64)
            if s_host.ndim == 1:
                s_host = s_host[:, None]
            if not np.all(np.isfinite(s_host)):
                raise ValueError("Input contains NaN or infinity (reference set s)")
            self._s_dev = torch.as_tensor(s_host).to(self.device)
            if (self._s_dev.dim() != 2 or self._s_dev.shape[1] != self._t_dev.shape[1]
                    or self._s_dev.shape[0] < 1):
                raise ValueError(f"reference set must be (nRef >= 1, {self._t_dev.shape[1]}), "
                                 f"got {tuple(self._s_dev.shape)}")

    def _init_wt(self):
        self.wt = np.copy(self.y)

    def _init_ws(self, k: int = 5):
        """5-NN uniform regression of y on t at s (nngp.py:45-47) on the GPU."""
        n = self._t_dev.shape[0]
        if n < k:
            raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {n}")
        idx = _lib.knn_query(self._t_dev, self._s_dev, k).long()
        y = torch.as_tensor(np.asarray(self.y, dtype=np.float64)).to(self.device)
        self.ws = y[idx].mean(dim=1).cpu().numpy()

    # -- per-axis ranges: the model is the isotropic one at phi = 1 on coordinates scaled column by column -------
    def _aniso_phi(self, cov: AnisotropicCovariance) -> tuple:
        if cov.dim != self._s_dev.shape[1]:
            raise ValueError(f"AnisotropicCovariance has {cov.dim} decays for {self._s_dev.shape[1]}-dimensional "
                             "coordinates (len(phi) must equal the coordinate dimension)")
        return cov.phi

    def _sep_model(self, cov: "SeparableCovariance") -> "SeparableCovariance":
        """``cov`` checked against this instance: S = T, 2 or 3 coordinate columns, 1 <= m <= 32."""
        if not self._same_sets():
            _refuse_sep(cov, f"refType={self.refType!r}")
        d = self._s_dev.shape[1]
        if d not in (2, 3):
            raise ValueError(f"a SeparableCovariance needs 2 or 3 coordinate columns (space, then time), got {d}")
        if not 1 <= self.m <= _lib.GRAD_MAX_M:
            raise NotImplementedError(f"the separable sweeps serve 1 <= m <= {_lib.GRAD_MAX_M} (m={self.m})")
        return cov

    def _metric_phi(self, cov):
        """The per-column scales of the neighbour search: an :class:`AnisotropicCovariance`'s decays, a
        :class:`SeparableCovariance`'s (phi_s, .., phi_s, phi_t), else None (the coordinates themselves)."""
        if isinstance(cov, AnisotropicCovariance):
            return self._aniso_phi(cov)
        if isinstance(cov, SeparableCovariance):
            return tuple(self._sep_model(cov).scaled(self._s_dev.shape[1]).tolist())
        return None

    def _phi_dev(self, phi) -> torch.Tensor:
        return torch.tensor(phi, dtype=torch.float64, device=self.device)

    def _scaled_s(self, phi) -> torch.Tensor:
        """``s * phi`` on the device: one buffer kept for the instance's life, rewritten in place when phi changes.
        The neighbour search and the sweeps share it, so the returned tensor is valid only until the next call with
        another phi: callers use it at once (launches are stream-ordered) and do not keep it."""
        buf = getattr(self, "_s_scaled", None)
        if buf is None:
            buf = self._s_scaled = torch.empty_like(self._s_dev)
            self._s_scaled_phi = None
        if self._s_scaled_phi != phi:
            torch.mul(self._s_dev, self._phi_dev(phi), out=buf)
            self._s_scaled_phi = phi
        return buf

    def _sweep_cov(self, cov=None):
        """``(covariance, reference coordinates)`` of a forward sweep: an :class:`AnisotropicCovariance` runs as
        its isotropic form at phi = 1 on the scaled copy of ``s``; every other form on ``s`` itself."""
        c = self.cov if cov is None else cov
        if isinstance(c, AnisotropicCovariance):
            return c.scaled()[0], self._scaled_s(self._aniso_phi(c))
        if isinstance(c, SeparableCovariance):  # its own fused sweeps, on the raw coordinates (_sweep_any)
            return self._sep_model(c), self._s_dev
        return self._covariance(c), self._s_dev

    def _query_scale(self, cov, q: torch.Tensor) -> torch.Tensor:
        c = self.cov if cov is None else cov
        return q * self._phi_dev(self._aniso_phi(c)) if isinstance(c, AnisotropicCovariance) else q

    def rebuild_neighbors(self, cov=None):
        """Rebuild the neighbour sets in the metric of ``cov`` (default ``self.cov``): the existing search on the
        coordinates scaled by an :class:`AnisotropicCovariance`'s decays or a :class:`SeparableCovariance`'s
        (phi_s, .., phi_s, phi_t) -- for a product correlation a heuristic: the scaled Euclidean distance does not order
        pairs by their correlation --, on the coordinates themselves for any other covariance.  Clears the kept
        factors and covariance blocks."""
        c = self.cov if cov is None else cov
        self._nbr_phi = self._metric_phi(c)
        self._make_s_neighbor_sets()
        self._make_t_neighbor_sets()
        self._B = self._F = None
        self._blk_cache = None
        self._latent = self._latent_ref = self._factor = None

    def _nbr_coords(self, x: torch.Tensor, own: bool = False) -> torch.Tensor:
        """``x`` in the neighbour search's metric (``own``: x is ``s`` itself, whose scaled copy is kept)."""
        if self._nbr_phi is None:
            return x
        return self._scaled_s(self._nbr_phi) if own else x * self._phi_dev(self._nbr_phi)

    def _make_s_neighbor_sets(self):
        self.nbr = _lib.knn_prior(self._nbr_coords(self._s_dev, True), self.m)  # int32 (N, m), -1 padded
        # Z-order visiting order + neighbour rows in that order, for the sweeps (speed only)
        self._order, self._nbr_sorted = _lib.row_order(self._s_dev, nbr=self.nbr)
        self._Ns = None

    def set_neighbor_sets(self, nbr: torch.Tensor):
        """Replace the neighbour sets (int32 (N, m) device tensor, -1 padded, prior indices)."""
        if nbr.shape != self.nbr.shape or nbr.dtype != torch.int32:
            raise ValueError(f"nbr must be int32 {tuple(self.nbr.shape)}")
        self.nbr = nbr.to(self.device).contiguous()
        self._order, self._nbr_sorted = _lib.row_order(self._s_dev, nbr=self.nbr)
        self._Ns = None
        self._B = self._F = None
        self._blk_cache = None

    def _make_t_neighbor_sets(self):
        """'S=T': Nt aliases Ns (nngp.py:65-67); otherwise the m nearest points of S to
        every t (nngp.py:68-71), ascending, on the GPU (nngp_knn_query)."""
        self._Nt = None
        if self._same_sets():
            self.nbr_t = None
            return
        k = min(self.m, self._s_dev.shape[0])
        self.nbr_t = _lib.knn_query(self._nbr_coords(self._s_dev, True), self._nbr_coords(self._t_dev), k) \
            if k > 0 else torch.empty(
            (self._t_dev.shape[0], 0), dtype=torch.int32, device=self.device)

    def _same_sets(self) -> bool:
        return isinstance(self.refType, str) and self.refType == "S=T"

    @property
    def Ns(self):
        """Reference format: list with ``Ns[0] == []`` and int64 arrays of min(i, m) indices."""
        if self._Ns is None:
            a = self.nbr.cpu().numpy().astype(np.int64)
            ns = [[]]
            for i in range(1, a.shape[0]):
                ns.append(a[i, : min(i, self.m)])
            self._Ns = ns
        return self._Ns

    @property
    def Nt(self):
        """'S=T': the same object as ``Ns``; otherwise one int64 index array into ``s`` per t."""
        if self._same_sets():
            return self.Ns
        if self._Nt is None:
            a = self.nbr_t.cpu().numpy().astype(np.int64)
            self._Nt = [row for row in a]
        return self._Nt

    # -- prediction at t ------------------------------
    # -- per-point noise in the response model ---------------------------------
    def _noise_sigmas(self, e, n: int, what: str, positive: bool) -> torch.Tensor:
        """``n`` per-point sigmas as the device weights v = e^2 (finite; positive, or >= 0 for an explicit array)."""
        e = e.detach().cpu().numpy() if isinstance(e, torch.Tensor) else e
        e = None if e is None else np.asarray(e, dtype=np.float64)
        if e is None or e.shape != (n,):
            raise ValueError(f"{what} must hold one sigma per location ({n},), got "
                             f"{'None' if e is None else e.shape}")
        if not np.all(np.isfinite(e)) or np.any(e <= 0 if positive else e < 0):
            raise ValueError(f"{what} must be finite and {'positive' if positive else 'non-negative'}")
        return torch.from_numpy(e * e).to(self.device)

    def _noise_setup(self, noise, cov=None):
        """``noise=`` of the response-model methods: ``(cv, v)`` with ``cv`` the fused-kind :class:`Covariance` and
        ``v`` the device weights (noise variance tau2 v_i).  ``"eps"``: the instance's per-location sigmas, as
        :meth:`oneSample` and :meth:`latent_posterior` read them; an array: sigmas in model order."""
        if not self._same_sets():
            _refuse_noise(f"refType={self.refType!r}")
        c = self.cov if cov is None else cov
        _refuse_sep(c, "per-point noise (noise=)")
        if isinstance(c, AnisotropicCovariance):
            _refuse_noise("an AnisotropicCovariance")
        if not isinstance(c, Covariance):
            _refuse_noise(f"a callable or custom covariance ({type(c).__name__})")
        if c.kind == "matern":
            _refuse_noise("the general-nu matern kind")
        if not 1 <= self.m <= _lib.GRAD_MAX_M:
            _refuse_noise(f"m={self.m}")
        if isinstance(noise, _NoiseVar):
            return c, noise.v
        n = self.nbr.shape[0]
        if isinstance(noise, str):
            if noise != "eps":
                raise ValueError(f"noise must be None, 'eps' or an array of sigmas, got {noise!r}")
            return c, self._noise_sigmas(self.eps, n, "noise='eps': the instance's eps", positive=True)
        return c, self._noise_sigmas(noise, n, "noise", positive=False)

    def predict(self, values=None, cov: Optional[Covariance] = None, query=None, algo: str = "auto", X=None,
                X_query=None, noise=None, noise_query=None):
        """Kriging of the NNGP at the points ``query`` (default ``t``) from ``values`` on S
        (default ``ws``): returns numpy ``(mean, var)`` with mean_t = B_t v_N(t) and
        var_t = F_t (conditional variance; includes tau2 like C_tt = sigma2 + tau2).
        Neighbours: the m nearest points of S to each query point (for query = t with
        refType != 'S=T' these are ``Nt``).

        ``X`` (n, p) and ``X_query`` (n_query, p): universal kriging of ``values`` (default ``y``) with the
        regression mean X beta, beta by GLS at ``cov`` (:meth:`gls`): mean x_q' beta + B_q (y - X beta)_N and
        variance F_q + h_q' cov_beta h_q, h_q = x_q - B_q X_N (``pynngp_amd.regression.universal_kriging``).

        ``noise`` (``"eps"`` or sigmas e in model order): the reference points' noise variances are tau2 e_j^2 in
        the neighbour blocks (``nngp_bf_cross_noise``); ``noise_query`` (n_query,) sigmas set the predicted points' own
        noise variance (default 1: var_t includes tau2).  ``algo`` is not used then."""
        if (X is None) != (X_query is None):
            raise ValueError("universal kriging needs both X and X_query")
        if noise is None and noise_query is not None:
            raise ValueError("noise_query needs noise")
        if noise is not None and X is not None:
            _refuse_noise("universal kriging (X, X_query)")
        nzv = None if noise is None else self._noise_setup(noise, cov)[1]
        if X is not None:
            from . import regression

            _refuse_sep(self.cov if cov is None else cov, "universal kriging (predict with X, X_query)")
            mean, var, _ = regression.universal_kriging(self, cov, X, X_query, values=values, query=query, algo=algo)
            return mean, var
        cv, sc = self._sweep_cov(cov)
        v = self.ws if values is None else values
        v = torch.as_tensor(np.asarray(v, dtype=np.float64) if not isinstance(v, torch.Tensor) else v,
                            dtype=torch.float64).to(self.device)
        if v.shape != (self._s_dev.shape[0],):
            raise ValueError(f"values must have one entry per reference point ({self._s_dev.shape[0]})")
        if query is None and not self._same_sets():
            q, nbr = self._t_dev, self.nbr_t
        else:
            q = self._t_dev if query is None else torch.as_tensor(
                np.ascontiguousarray(query, dtype=np.float64)).to(self.device)
            k = min(self.m, self._s_dev.shape[0])
            nbr = None
        q = self._query_scale(cov, q)  # an AnisotropicCovariance: the query points in the scaled coordinates too
        if nbr is None and isinstance(cv, SeparableCovariance):
            # the search in the (phi_s, .., phi_s, phi_t) metric, the cross sweep on the coordinates themselves
            ph = self._metric_phi(cv)
            nbr = _lib.knn_query(self._scaled_s(ph), q * self._phi_dev(ph), k)
        if nbr is None:
            nbr = _lib.knn_query(sc, q, k)
        n = q.shape[0]
        if nbr.shape[1] == 0:  # m = 0: the marginal
            if isinstance(cv, Covariance):
                return np.zeros(n), np.full(n, cv.sigma2 + cv.tau2)
            return np.zeros(n), cv.marginal(q).cpu().numpy()
        if nzv is not None:
            nq = None if noise_query is None else self._noise_sigmas(noise_query, n, "noise_query", positive=False)
            _, F, R, p = _lib.bf_cross_noise(sc, q, nbr, cv.kind, *cv.theta[:3], nzv, noise_query=nq, ref_values=v,
                                             want_r=True)
            _raise_on_bad(p.cpu().numpy())
            return (-R).cpu().numpy(), F.cpu().numpy()
        R = torch.empty(n, dtype=torch.float64, device=self.device)
        _, F, p = _sweep_any(cv, sc, nbr, 0, values=v, algo=algo, R=R, qcoords=q)
        _raise_on_bad(p.cpu().numpy(), cv)
        return (-R).cpu().numpy(), F.cpu().numpy()

    # -- covariance plumbing ---------------------------------------------------
    def _covariance(self, cov=None):
        """The covariance the device sweeps use: ``cov`` (default ``self.cov``); a plain callable
        ``cov(a, b)`` becomes a :class:`CallableCovariance` (one per callable, so its evaluation mode
        is probed once)."""
        c = self.cov if cov is None else cov
        _refuse_aniso(c, "this method")
        if isinstance(c, (Covariance, IsotropicCovariance, CallableCovariance)):
            return c
        if c is None or not callable(c):
            raise TypeError("the device B/F sweep needs a covariance: pynngp_amd.Covariance(kind, sigma2, phi, tau2[, "
                            f"nu]), IsotropicCovariance(fn, tau2) or a callable cov(a, b) (got {type(c).__name__})")
        wrapped = getattr(self, "_wrapped_cov", None)
        if wrapped is None or wrapped.fn is not c:
            wrapped = CallableCovariance(c)
            self._wrapped_cov = wrapped
        return wrapped

    def _field_blocks(self, cv):
        """Joint blocks of the whole field (Z-order rows) for a :class:`CallableCovariance` (None for the
        other covariance forms).  Evaluating them is the caller's code and the most expensive step; with
        ``CallableCovariance(fn, cache=True)`` they are kept for the next sweep (8 (m+1)(m+2)/2 bytes per
        location of device memory), keyed on the object, its nugget and the neighbour sets
        (:meth:`clear_cache` drops them); by default every sweep evaluates the plug-in again, as the
        reference calls ``cov`` on every evaluation (advice r04: a mutable plug-in must not see stale
        blocks)."""
        if not isinstance(cv, CallableCovariance):
            return None
        hit = getattr(self, "_blk_cache", None)
        if cv.cache and hit is not None and hit[0] is cv and hit[1] is self._nbr_sorted and hit[2] == cv.tau2:
            return hit[3]
        self._blk_cache = None
        blk = cv.blocks(self._s_dev, self._nbr_sorted, 0, order=self._order)
        if cv.cache:
            self._blk_cache = (cv, self._nbr_sorted, cv.tau2, blk)
        return blk

    def clear_cache(self):
        """Drop kept covariance blocks and factors (a cached plug-in's parameters changed)."""
        self._blk_cache = None
        self._B = self._F = None

    def _nbr_idx(self, i):
        row = self.nbr[i]
        return row[row >= 0].long()

    def _call_cov(self, a, b):
        if self.cov is None:
            raise TypeError("cov is None")
        if isinstance(self.cov, (Covariance, AnisotropicCovariance, IsotropicCovariance)):
            return self.cov(a, b)
        return self.cov(a.cpu().numpy(), b.cpu().numpy())  # the reference's rows are numpy (nngp.py:7,31)

    # -- per-location algebra (nngp.py:73-96) ----------------------------------
    def _CNs(self, i):
        """C_{N(s_i)} (nngp.py:78-82), with the nugget on the diagonal for a Covariance."""
        x = self._s_dev[self._nbr_idx(i)]
        c = self._call_cov(x, x)
        if isinstance(self.cov, (Covariance, AnisotropicCovariance, IsotropicCovariance)) and self.cov.tau2 > 0:
            c = c + self.cov.tau2 * torch.eye(x.shape[0], dtype=c.dtype, device=c.device)
        return c.cpu().numpy() if isinstance(c, torch.Tensor) else c

    def _Ccross(self, i):
        """C_{s_i, N(s_i)} (nngp.py:84-86), shape (1, k)."""
        c = self._call_cov(self._s_dev[i][None, :], self._s_dev[self._nbr_idx(i)])
        return c.cpu().numpy() if isinstance(c, torch.Tensor) else c

    def _Cs(self, i):
        """C_{s_i, s_i} (nngp.py:92-96), with the nugget for a Covariance."""
        x = self._s_dev[i][None, :]
        c = self._call_cov(x, x)
        if isinstance(self.cov, (Covariance, AnisotropicCovariance, IsotropicCovariance)):
            c = c + self.cov.tau2
        return c.cpu().numpy() if isinstance(c, torch.Tensor) else c

    def _row_bf(self, i):
        cv, sc = self._sweep_cov()
        B, F, p = _sweep_any(cv, sc, self.nbr[i: i + 1], int(i))
        _raise_on_bad(p.cpu().numpy(), cv)
        k = min(int(i), self.m)
        return B[0, :k].cpu().numpy(), float(F[0].item())

    def _Bsi(self, i):
        """B_{s_i} = C_{s_i,N} C_N^{-1} (nngp.py:73-76) from the device kernel."""
        return self._row_bf(i)[0]

    def _Fsi(self, i):
        """F_{s_i} = C_ii - B_i C_{N,s_i} (nngp.py:88-90) from the device kernel."""
        return self._row_bf(i)[1]

    # -- whole-field sweep -----------------------------------------------------
    def compute_BF(self, algo: str = "auto"):
        """All B (N, m) and F (N,) as device tensors (one fused sweep)."""
        cv, sc = self._sweep_cov()
        B, F, p = _sweep_any(cv, sc, self._nbr_sorted, 0, algo=algo, order=self._order,
                             blocks=self._field_blocks(cv))
        _raise_on_bad(p.cpu().numpy(), cv)
        self._B, self._F = B, F
        return B, F

    @property
    def B(self):
        return self.compute_BF()[0] if self._B is None else self._B

    @property
    def F(self):
        return self.compute_BF()[1] if self._F is None else self._F

    def loglik(self, values=None, cov: Optional[Covariance] = None, algo: str = "auto", noise=None) -> float:
        """NNGP log density of ``values`` (default ``y``): -1/2 sum [log 2pi + log F + r^2/F].

        ``noise``: ``"eps"`` (the instance's per-location sigmas) or an array of sigmas e in model order: the noise
        variance of point i is tau2 e_i^2 instead of tau2 (``nngp_bf_sweep_noise``; ``algo`` is not used then)."""
        if noise is not None:
            cv, nzv = self._noise_setup(noise, cov)
            v = self._values_dev(values)
            _, _, _, p = _lib.bf_sweep_noise(self._s_dev, self._nbr_sorted, 0, cv.kind, *cv.theta[:3], nzv, values=v,
                                             want_bf=False, order=self._order)
            ph = p.cpu().numpy()
            _raise_on_bad(ph)
            return -0.5 * (self.nbr.shape[0] * LOG_2PI + ph[0] + ph[1])
        cv, sc = self._sweep_cov(cov)
        v = self.y if values is None else values
        v = torch.as_tensor(np.asarray(v, dtype=np.float64) if not isinstance(v, torch.Tensor) else v,
                            dtype=torch.float64).to(self.device)
        if v.dim() != 1 or v.shape[0] != self.nbr.shape[0]:
            raise ValueError(f"loglik needs one value per location ({self.nbr.shape[0]}, 1-D)")
        _, _, p = _sweep_any(cv, sc, self._nbr_sorted, 0, values=v, qvalues=v, want_bf=False, algo=algo,
                             order=self._order, blocks=self._field_blocks(cv))
        ph = p.cpu().numpy()
        _raise_on_bad(ph, cv)
        n = self.nbr.shape[0]
        return -0.5 * (n * LOG_2PI + ph[0] + ph[1])

    def gls(self, cov: Optional[Covariance], X, values=None, reml: bool = False, algo: str = "auto", noise=None):
        """GLS of ``values`` (default y) on the design ``X`` (n, p; p + 1 <= 16; the caller adds the intercept
        column) under the NNGP precision at ``cov``: one sweep that writes B and F, then one ``nngp_whiten_gram`` on
        [y, X]; the p x p algebra on the host.  Returns a :class:`pynngp_amd.regression.GLSResult` (``beta``,
        ``cov_beta``, ``loglik``, ``reml``, ``gram``); with ``reml=True`` its ``objective`` is the restricted
        likelihood, else the profile likelihood.  A rank-deficient ``X`` raises :class:`NNGPNumericalError`."""
        from . import regression

        if noise is not None:
            _refuse_noise("gls (a regression mean)")
        if reml:
            _refuse_sep(self.cov if cov is None else cov, "the restricted likelihood (reml=True)")
        return regression.gls(self, cov, X, values=values, reml=reml, algo=algo)

    def conjugate(self, kind: str, phi: float, alpha: float, X, prior: Optional[dict] = None,
                  nu: Optional[float] = None, values=None, algo: str = "auto", noise=None):
        """The conjugate NNGP (Finley et al.; spNNGP's ``spConjNNGP``) of ``values`` (default y) on ``X`` at fixed
        (phi, alpha = tau2 / sigma2), computed at ``Covariance(kind, 1, phi, alpha)``: beta and sigma2 integrate out
        in closed form.  ``prior``: dict ``a``, ``b`` (sigma2 ~ IG(a, b), default 2, 1) and optionally ``mu``, ``V``
        (beta | sigma2 ~ N(mu, sigma2 V); default flat).  Returns a :class:`pynngp_amd.regression.ConjugateNNGP`: the
        Normal-inverse-gamma posterior ``mu``, ``V``, ``a``, ``b``, ``log_evidence`` = log p(y | phi, alpha), and
        ``predict(query, X_query)``, the Student-t predictive (location, scale, 2 a degrees of freedom)."""
        from . import regression

        if noise is not None:
            _refuse_noise("conjugate")
        _refuse_aniso(self.cov, "conjugate")
        return regression.conjugate(self, kind, phi, alpha, X, prior=prior, nu=nu, values=values, algo=algo)

    def conjugate_grid(self, phis, alphas, kind: str, X, prior: Optional[dict] = None, nu: Optional[float] = None,
                       values=None, algo: str = "auto"):
        """:meth:`conjugate` over a grid: dict with ``log_evidence`` (len(phis), len(alphas)), its argmax ``phi`` /
        ``alpha`` and ``best``, the fit there."""
        from . import regression

        _refuse_aniso(self.cov, "conjugate_grid")
        return regression.conjugate_grid(self, phis, alphas, kind, X, prior=prior, nu=nu, values=values, algo=algo)

    def profile_loglik(self, cov: Covariance, values=None, mean: str = "constant", algo: str = "auto", X=None,
                       noise=None):
        """NNGP log-likelihood of ``values`` (default y) at ``cov`` with a constant mean
        profiled out by GLS under the NNGP precision (I - B)^T F^-1 (I - B):
        mu = sum(r1 ry / F) / sum(r1^2 / F), r1 = (I - B) 1, ry = (I - B) y (two fused
        sweeps with residual output).  ``mean="zero"`` is :meth:`loglik`.  Returns
        ``(loglik, mu)``.  ``mean="linear"`` with ``X`` (n, p): the regression mean X beta profiled out
        (:meth:`gls`: one sweep and one whitened Gram); returns ``(loglik, beta)``.  ``noise``: as :meth:`loglik`
        (constant and zero means)."""
        if noise is not None and (mean == "linear" or X is not None):
            _refuse_noise("mean='linear'")
        if mean == "linear":
            if X is None:
                raise ValueError("mean='linear' needs the design matrix X")
            res = self.gls(cov, X, values=values, algo=algo)
            return res.loglik, res.beta
        if X is not None:
            raise ValueError("X is the design of mean='linear'")
        v = self.y if values is None else values
        v = torch.as_tensor(np.asarray(v, dtype=np.float64) if not isinstance(v, torch.Tensor) else v,
                            dtype=torch.float64).to(self.device)
        if mean == "zero":
            return self.loglik(v, cov, algo, noise=noise), 0.0
        if mean != "constant":
            raise ValueError("mean must be 'constant', 'zero' or 'linear'")
        n = v.shape[0]
        if noise is not None:
            cv, nzv = self._noise_setup(noise, cov)
            v = self._values_dev(v)
            kw = dict(want_bf=True, want_r=True, order=self._order)
            _, F, ry, py = _lib.bf_sweep_noise(self._s_dev, self._nbr_sorted, 0, cv.kind, *cv.theta[:3], nzv, values=v,
                                               **kw)
            _, _, r1, p1 = _lib.bf_sweep_noise(self._s_dev, self._nbr_sorted, 0, cv.kind, *cv.theta[:3], nzv,
                                               values=torch.ones_like(v), **kw)
            sums = torch.stack([py[0], py[1], p1[1], torch.sum(ry * r1 / F), py[2], py[3]]).cpu().numpy()
            _raise_on_bad(np.array([0.0, 0.0, sums[4], sums[5]]))
            logF, qyy, q11, qy1 = sums[:4]
            mu = qy1 / q11
            return -0.5 * (n * LOG_2PI + logF + qyy - 2.0 * mu * qy1 + mu * mu * q11), float(mu)
        ry = torch.empty(n, dtype=torch.float64, device=self.device)
        r1 = torch.empty_like(ry)
        cov, sc = self._sweep_cov(cov)
        kw = dict(algo=algo, order=self._order, blocks=self._field_blocks(cov))
        _, F, py = _sweep_any(cov, sc, self._nbr_sorted, 0, values=v, qvalues=v, R=ry, **kw)
        ones = torch.ones_like(v)
        _, _, p1 = _sweep_any(cov, sc, self._nbr_sorted, 0, values=ones, qvalues=ones, R=r1, **kw)
        s_y1 = torch.sum(ry * r1 / F)
        sums = torch.stack([py[0], py[1], p1[1], s_y1, py[2], py[3]]).cpu().numpy()
        _raise_on_bad(np.array([0.0, 0.0, sums[4], sums[5]]), cov)
        logF, qyy, q11, qy1 = sums[:4]
        mu = qy1 / q11
        quad = qyy - 2.0 * mu * qy1 + mu * mu * q11
        return -0.5 * (n * LOG_2PI + logF + quad), float(mu)

    def _grad_cov(self, cov, aniso: bool = True):
        """The covariance of a gradient sweep: a fused kind other than the general-nu Matern, m >= 1."""
        cv = self.cov if cov is None else cov
        if isinstance(cv, SeparableCovariance):
            if not aniso:
                _refuse_sep(cv, "the Fisher information (fisher_information, fit(method='fisher'), stderr=True)")
            return self._sep_model(cv)
        if isinstance(cv, AnisotropicCovariance):
            self._aniso_phi(cv)
        else:
            cv = self._covariance(cov)
        if not isinstance(cv, (Covariance, AnisotropicCovariance)):
            raise TypeError("the analytic gradient needs a Covariance of a fused kind (exponential, matern32, "
                            f"matern52, gaussian, spherical), not {type(cv).__name__}")
        if not aniso:
            _refuse_aniso(cv, "the Fisher information (fisher_information, fit(method='fisher'), stderr=True)")
        if cv.kind == "matern" and not (aniso and isinstance(cv, MaternCovariance)):
            raise NotImplementedError("the analytic gradient does not serve the general-nu matern kind")
        if not 1 <= self.m <= _lib.GRAD_MAX_M:
            raise NotImplementedError(f"the analytic gradient serves 1 <= m <= {_lib.GRAD_MAX_M} (m={self.m})")
        return cv

    def _matern_grad_ws(self) -> torch.Tensor:
        """The Matern gradient sweep's workspace (records and tables), kept across a fit's evaluations."""
        need = _lib.load().nngp_bf_grad_matern_workspace_bytes(self.nbr.shape[0], self.m)
        ws = getattr(self, "_mgrad_ws", None)
        if ws is None or ws.numel() < need or ws.device != self._s_dev.device:
            ws = self._mgrad_ws = _lib._workspace(need, self._s_dev.device)
        return ws

    def _values_dev(self, values):
        v = self.y if values is None else values
        v = torch.as_tensor(np.asarray(v, dtype=np.float64) if not isinstance(v, torch.Tensor) else v,
                            dtype=torch.float64).to(self.device)
        if v.dim() != 1 or v.shape[0] != self.nbr.shape[0]:
            raise ValueError(f"one value per location is needed ({self.nbr.shape[0]}, 1-D)")
        return v

    def loglik_grad(self, values=None, cov: Optional[Covariance] = None, noise=None):
        """:meth:`loglik` and its analytic gradient in (sigma2, phi, tau2) from one fused gradient sweep
        (``nngp_bf_grad``): ``(loglik, grad)`` with ``grad`` a float64 ndarray (3,).  An
        :class:`AnisotropicCovariance` gives the gradient in (sigma2, phi_1 .. phi_dim, tau2), (dim + 2,), from one
        ``nngp_bf_grad_aniso`` sweep on the raw coordinates; a :class:`MaternCovariance` the gradient in
        (sigma2, phi, tau2, nu), (4,), from one ``nngp_bf_grad_matern`` sweep.  ``noise``: as :meth:`loglik`, the
        gradient in (sigma2, phi, tau2) from one ``nngp_bf_grad_noise`` sweep (tau2 scales the given variances)."""
        if noise is not None:
            cv, nzv = self._noise_setup(noise, cov)
            p, g, _ = _lib.bf_grad_noise(self._s_dev, self._nbr_sorted, 0, cv.kind, *cv.theta[:3],
                                         self._values_dev(values), nzv, order=self._order)
            h = torch.cat([p, g]).cpu().numpy()
            _raise_on_bad(h[:4])
            return -0.5 * (self.nbr.shape[0] * LOG_2PI + h[0] + h[1]), h[4:7].copy()
        cv = self._grad_cov(cov)
        v = self._values_dev(values)
        if isinstance(cv, SeparableCovariance):  # (sigma2, phi_s, phi_t, tau2) from one nngp_bf_grad_sep sweep
            p, g, _ = _lib.bf_grad_sep(self._s_dev, self._nbr_sorted, 0, cv.kind_s, cv.kind_t, *cv.theta, v,
                                       order=self._order)
            h = torch.cat([p, g]).cpu().numpy()
            _raise_on_bad(h[:4], cv)
            return -0.5 * (self.nbr.shape[0] * LOG_2PI + h[0] + h[1]), h[4:].copy()
        if isinstance(cv, MaternCovariance):
            p, g, _ = _lib.bf_grad_matern(self._s_dev, self._nbr_sorted, 0, cv.sigma2, cv.phi, cv.tau2, cv.nu, v,
                                          order=self._order, workspace=self._matern_grad_ws())
            h = torch.cat([p, g]).cpu().numpy()
            _raise_on_bad(h[:4])
            return -0.5 * (self.nbr.shape[0] * LOG_2PI + h[0] + h[1]), h[4:].copy()
        if isinstance(cv, AnisotropicCovariance):
            p, g, _ = _lib.bf_grad_aniso(self._s_dev, self._nbr_sorted, 0, cv.kind, cv.sigma2, cv.phi, cv.tau2, v,
                                         order=self._order)
            h = torch.cat([p, g]).cpu().numpy()
            _raise_on_bad(h[:4])
            return -0.5 * (self.nbr.shape[0] * LOG_2PI + h[0] + h[1]), h[4:].copy()
        p, g, _ = _lib.bf_grad(self._s_dev, self._nbr_sorted, 0, cv.kind, cv.sigma2, cv.phi, cv.tau2, v,
                               order=self._order)
        h = torch.cat([p, g]).cpu().numpy()
        _raise_on_bad(h[:4])
        n = self.nbr.shape[0]
        return -0.5 * (n * LOG_2PI + h[0] + h[1]), h[4:7].copy()

    def profile_loglik_grad(self, cov: Covariance, values=None, mean: str = "constant", X=None, noise=None):
        """:meth:`profile_loglik` and its gradient in (sigma2, phi, tau2): ``(loglik, mu, grad)``.  By the
        envelope theorem the gradient of the profiled likelihood is the plain gradient at ``values - mu``:
        the two sweeps for mu plus one gradient sweep.  ``mean="linear"`` with ``X``: ``(loglik, beta, grad)``, the
        gradient sweep at ``values - X beta``.  ``noise``: as :meth:`loglik_grad` (constant and zero means)."""
        if noise is not None:
            if mean == "linear" or X is not None:
                _refuse_noise("mean='linear'")
            cv, nzv = self._noise_setup(noise, cov)
            nz = _NoiseVar(nzv)
            v = self._values_dev(values)
            if mean == "zero":
                ll, g = self.loglik_grad(v, cv, noise=nz)
                return ll, 0.0, g
            ll, mu = self.profile_loglik(cv, v, mean=mean, noise=nz)
            return ll, mu, self.loglik_grad(v - mu, cv, noise=nz)[1]
        cv = self._grad_cov(cov)
        v = self._values_dev(values)
        if mean == "linear":
            from . import regression

            ll, beta = self.profile_loglik(cv, v, mean="linear", X=X)
            Xd = regression.design(self, X, v.shape[0])
            return ll, beta, self.loglik_grad(v - Xd @ torch.from_numpy(beta).to(self.device), cv)[1]
        if X is not None:
            raise ValueError("X is the design of mean='linear'")
        if mean == "zero":  # one gradient sweep gives both
            ll, g = self.loglik_grad(v, cv)
            return ll, 0.0, g
        ll, mu = self.profile_loglik(cv, v, mean=mean)
        return ll, mu, self.loglik_grad(v - mu, cv)[1]

    def _fisher_sweep(self, cv: Covariance, v, want_rows: bool = False):
        """One ``nngp_bf_fisher`` sweep at ``cv`` over ``v`` (a device tensor, or None for the information alone):
        ``(loglik or None, grad (3,), info (3, 3), I_rows, G)``, host arrays but for the two row tensors."""
        from . import fisher

        p, g, info, I_rows, G = _lib.bf_fisher(self._s_dev, self._nbr_sorted, 0, cv.kind, cv.sigma2, cv.phi, cv.tau2,
                                               v, want_rows=want_rows, order=self._order)
        h = torch.cat([p, g, info]).cpu().numpy()
        _raise_on_bad(h[:4])
        n = self.nbr.shape[0]
        ll = None if v is None else -0.5 * (n * LOG_2PI + h[0] + h[1])
        return ll, h[4:7].copy(), fisher.info_matrix(h[7:13]), I_rows, G

    def fisher_information(self, cov: Optional[Covariance] = None, values=None, mean: str = "zero", X=None,
                           log: bool = False, rows: bool = False, noise=None) -> dict:
        """(``noise``: refused -- the information sweep has no per-point noise form.)  The Fisher information of the NNGP (Vecchia) likelihood in theta = (sigma2, phi, tau2) at ``cov``, from
        one fused sweep (``nngp_bf_fisher``): the sum over locations of each one's expected information under the
        exact Gaussian law of its joint block (Guinness 2021), positive semi-definite by construction.

        Returns a dict with ``info`` (3, 3), ``grad`` (3,) and ``loglik``; with a profiled mean also ``mu``
        (``mean="constant"``) or ``beta`` (``mean="linear"`` with ``X``), the gradient and likelihood then taken at
        ``values - mean`` as in :meth:`profile_loglik_grad` (theta and the mean's coefficients are orthogonal in the
        information; the coefficients' own block is ``gls``'s ``gram``).  ``rows=True`` adds ``I_rows`` (n, 6), the
        locations' terms in the order (ss, sp, st, pp, pt, tt), and ``G`` (n, 3).  ``log=True`` gives the forms in log
        theta: diag(theta) I diag(theta) and theta * grad.

        ``values=None`` is the design-stage call: the information does not depend on the data, ``grad`` is exactly
        0 and ``loglik`` is None (``mean`` must then be ``"zero"``).  Fused kinds other than ``matern`` and
        1 <= m <= 32 only."""
        if noise is not None:
            _refuse_noise("the Fisher information (fisher_information, fit(method='fisher'), stderr=True)")
        from . import fisher

        cv = self._grad_cov(cov, aniso=False)
        if mean not in ("zero", "constant", "linear"):
            raise ValueError("mean must be 'constant', 'zero' or 'linear'")
        if mean == "linear" and X is None:
            raise ValueError("mean='linear' needs the design matrix X")
        if mean != "linear" and X is not None:
            raise ValueError("X is the design of mean='linear'")
        out = {}
        if values is None:
            if mean != "zero":
                raise ValueError("profiling a mean needs values: the design-stage call (values=None) takes mean='zero'")
            v = None
        else:
            v = self._values_dev(values)
            if mean == "linear":
                from . import regression

                _, beta = self.profile_loglik(cv, v, mean="linear", X=X)
                v = v - regression.design(self, X, v.shape[0]) @ torch.from_numpy(beta).to(self.device)
                out["beta"] = beta
            elif mean == "constant":
                _, mu = self.profile_loglik(cv, v, mean="constant")
                v = v - mu
                out["mu"] = mu
        ll, g, info, I_rows, G = self._fisher_sweep(cv, v, want_rows=rows)
        th = np.array(cv.theta[:3], dtype=np.float64)
        if log:
            info, g = fisher.to_log(info, g, th)
        out.update(info=info, grad=g, loglik=ll)
        if rows:
            I_rows, G = I_rows.cpu().numpy(), G.cpu().numpy()
            out.update(I_rows=fisher.info_rows_scale(I_rows, th) if log else I_rows, G=G * th if log else G)
        return out

    def _fit_stderr(self, kind, theta, nu, mean, X, free_tau: bool) -> dict:
        """``info``, ``cov_theta`` and ``se`` of a fit at ``theta``: one information sweep (the information does
        not read the data) and the inverse of the free parameters' block."""
        from . import fisher

        _, _, info, _, _ = self._fisher_sweep(self._grad_cov(Covariance(kind, *theta, nu=nu)), None)
        k = 3 if free_tau else 2
        cov_theta, se = fisher.theta_cov(info[:k, :k])
        return {"info": info[:k, :k].copy(), "cov_theta": cov_theta, "se": se}

    def _fit_fisher(self, kind, th0, nu, mean, X, linear, free_tau, fix_tau2, maxiter, tol, algo) -> dict:
        """Fisher scoring on the free log-parameters (:mod:`pynngp_amd.fisher` has the iteration and its ridge
        rule): each iteration profiles the mean, runs one information sweep at the residual and halves the step
        while the profiled likelihood falls."""
        from . import fisher

        k = 3 if free_tau else 2
        y = self._values_dev(None)
        state = {}

        def theta_of(z):
            return (math.exp(z[0]), math.exp(z[1]), math.exp(z[2]) if free_tau else float(fix_tau2))

        def profile(z):
            th = theta_of(z)
            cv = Covariance(kind, *th, nu=nu)
            try:
                if linear:
                    res = self.gls(cv, X, algo=algo)
                    return res.loglik, res.beta, cv
                ll, mu = self.profile_loglik(cv, mean=mean, algo=algo)
                return ll, mu, cv
            except NNGPNumericalError:
                return None

        def loglik_only(z):
            p = profile(z)
            return None if p is None else p[0]

        def evaluate(z):
            p = profile(z)
            if p is None:
                return None
            ll, mu, cv = p
            try:
                if linear:
                    v = y - X @ torch.from_numpy(mu).to(self.device)
                else:
                    v = y - mu if mean == "constant" else y
                _, g, info, _, _ = self._fisher_sweep(cv, v)
            except NNGPNumericalError:
                return None
            th = np.array(cv.theta[:3])
            I_log, g_log = fisher.to_log(info, g, th)
            state[tuple(z)] = (None if linear else mu, cv.theta[:3], info)
            return ll, g_log[:k], I_log[:k, :k]

        z0 = [math.log(th0[0]), math.log(th0[1])] + ([math.log(max(th0[2], 1e-6))] if free_tau else [])
        try:
            res = fisher.fisher_scoring(evaluate, z0, loglik_only=loglik_only, maxiter=maxiter,
                                        tol=fisher.DEFAULT_TOL if tol is None else tol)
        except FloatingPointError as e:
            raise NNGPNumericalError(f"Fisher scoring: {e}") from None
        mu, theta, info = state[tuple(res["z"])]
        theta = tuple(float(t) for t in theta)
        self.cov = Covariance(kind, *theta, nu=nu)
        self._B = self._F = None
        cov_theta, se = fisher.theta_cov(info[:k, :k])
        return {"theta": theta, "mu": mu, "loglik": res["loglik"], "n_evals": res["n_evals"] + res["n_loglik_evals"],
                "converged": res["converged"], **self._fit_beta(X if linear else None, algo), "n_iter": res["n_iter"],
                "info": info[:k, :k].copy(), "cov_theta": cov_theta, "se": se}

    def fit(self, kind: Optional[str] = None, x0=None, mean: str = "constant", fix_tau2: Optional[float] = None,
            method: Optional[str] = None, maxiter: int = 400, algo: str = "auto", nu: Optional[float] = None,
            gradient: Optional[bool] = None, X=None, reml: bool = False, stderr: bool = False,
            tol: Optional[float] = None,
            anisotropic: bool = False, reneighbor: int = 0, estimate_nu: Optional[bool] = None,
            nu_bounds=(0.05, 50.0), noise=None):
        """Maximum-likelihood (sigma2, phi, tau2) of the NNGP response model on S = T, each
        objective evaluation one or two fused GPU sweeps (scipy.optimize on log-parameters).
        ``x0`` defaults to ``cov``'s theta; ``fix_tau2`` holds the nugget fixed (e.g. 0 for the
        latent model); ``nu`` the (fixed) smoothness of the ``matern`` kind, default ``cov``'s.
        Sets ``cov`` to the estimate and returns a dict with theta, mu, loglik and the
        optimizer's evaluation count.  ``method`` defaults to Nelder-Mead.

        ``gradient=True``: the objective also returns the analytic gradient
        (:meth:`profile_loglik_grad`, d/d log theta = theta d/d theta) and scipy runs with ``jac=True``,
        L-BFGS-B by default; fused kinds other than ``matern`` and 1 <= m <= 32 only.  The result gains
        ``n_grad_evals``.  ``gradient=None``, the default, is ``False`` for every model but one built with a
        :class:`SeparableCovariance` (last paragraph), where it is ``True``.

        ``mean="linear"`` with ``X`` (n, p): the regression mean X beta is profiled out (:meth:`gls`); the result
        gains ``beta`` and ``cov_beta`` at the estimate and ``mu`` is None.  ``reml=True`` (``mean="linear"``, or
        ``"constant"`` as the design of ones) maximises the restricted likelihood instead, derivative-free.

        ``method="fisher"``: Fisher scoring on the free log-parameters (Guinness 2021; :mod:`pynngp_amd.fisher`):
        each iteration profiles the mean, takes the gradient and the expected information from one
        ``nngp_bf_fisher`` sweep at the residual, and halves the step I^-1 g while the profiled likelihood falls; it
        stops when |g . step| < ``tol`` (default 1e-10) or after ``maxiter`` steps.  ``fix_tau2`` drops the nugget's
        row and column.  The result gains ``n_iter``, ``info`` (the free parameters' block of the information in
        theta), ``cov_theta`` (its inverse) and ``se`` (the root of that diagonal).  The kinds and m of
        ``gradient=True``; no ``reml``.

        ``stderr=True`` adds ``info``, ``cov_theta`` and ``se`` to any other method's result: one information
        sweep at the estimate (the same kinds and m).

        ``anisotropic=True``: one decay per coordinate axis (:class:`AnisotropicCovariance`), L-BFGS-B on the log of
        (sigma2, phi_1 .. phi_dim, tau2) with :meth:`profile_loglik_grad` (``nngp_bf_grad_aniso``).  ``x0`` =
        (sigma2, phi, tau2) with ``phi`` one number (used for every axis) or a tuple; ``fix_tau2`` and ``mean`` as
        above.  The analytic gradient is always used, whatever ``gradient`` says; ``method`` is any scipy method that
        takes ``jac``; ``tol`` is the gradient tolerance (L-BFGS-B's ``gtol``: it stops once no free log-parameter's
        derivative exceeds it; default scipy's 1e-5, beside scipy's relative-decrease rule ``ftol``); ``algo`` serves
        the sweeps that take one (the final ``beta`` and a reneighboured likelihood); ``nu`` is refused (no kind
        served here has one).  The result carries ``phi`` as a tuple, ``theta`` = (sigma2, *phi, tau2), ``grad``, the
        gradient in the free log-parameters at the optimiser's last iterate (all zeros, with ``converged`` False,
        when that iterate was not positive definite) and ``message``, the optimiser's stopping reason.
        ``reneighbor=r`` runs r further rounds: each calls :meth:`rebuild_neighbors` at the current estimate and
        restarts the optimiser from it (the likelihood of a round is the one on that round's sets).  No ``stderr``,
        ``method="fisher"`` or ``reml`` with it.

        ``estimate_nu`` (``kind="matern"`` only; None, the default, changes nothing): ``True`` runs L-BFGS-B on the
        log of (sigma2, phi, tau2, nu) from ``nu`` with the four-component gradient of one ``nngp_bf_grad_matern``
        sweep per evaluation (:class:`MaternCovariance`), nu kept inside ``nu_bounds``; ``False`` does the same at
        the fixed ``nu`` with the first three components.  ``fix_tau2`` and ``mean`` as for ``anisotropic=True``;
        ``tol`` is L-BFGS-B's ``gtol`` and, when given, the only stopping rule beside ``maxiter`` (``ftol`` is set
        to 1e-15).  The result carries ``nu``, ``theta`` = (sigma2, phi, tau2, nu), ``grad`` (the
        gradient in the free log-parameters at the optimiser's last iterate) and ``message``.  No ``reml``,
        ``anisotropic``, ``method="fisher"`` or ``stderr`` with it.

        ``noise`` (``"eps"`` or sigmas e in model order): per-point noise variances tau2 e_i^2 (:meth:`loglik`).
        ``fix_tau2=1.0`` takes the error bars as exact; a free tau2 rescales them.  Derivative-free or
        ``gradient=True`` (``nngp_bf_grad_noise``; ``tol``, when given, is then L-BFGS-B's ``gtol`` and the only
        stopping rule beside ``maxiter``); the result gains ``grad``, the gradient in the free log-parameters at the
        estimate.  Constant and zero means; no ``stderr``, ``method="fisher"``, ``anisotropic``, ``reml``,
        ``estimate_nu`` or the ``matern`` kind with it.

        A model built with a :class:`SeparableCovariance`: L-BFGS-B on the analytic gradient
        (``nngp_bf_grad_sep``) over the free log-parameters of (sigma2, phi_s, phi_t, tau2), the two kinds fixed to
        the model's.  ``x0`` = (sigma2, phi_s, phi_t, tau2) (default: the model's theta); ``fix_tau2``, ``mean``,
        ``X``, ``tol`` (L-BFGS-B's ``gtol``, then the only stopping rule beside ``maxiter``), ``maxiter`` and
        ``reneighbor=r`` as for ``anisotropic=True``.  ``gradient=None`` (the default) and ``True`` are this fit;
        ``gradient=False``: Nelder-Mead on the forward sweep.  The result carries ``theta``, ``grad`` (the gradient in
        the free log-parameters at the reported ``theta``), ``loglik``, ``n_evals``, ``n_grad_evals``, ``converged`` and
        ``message``.  A neighbour index out of range raises :class:`NNGPIndexError` from this model's methods: an
        ``NNGPNumericalError`` and an ``IndexError`` (what every other model raises) at once.
        Every other option raises ``TypeError``."""
        gradient_asked = gradient
        gradient = bool(gradient)
        if isinstance(getattr(self, "cov", None), SeparableCovariance):
            # a SeparableCovariance model: L-BFGS-B on the analytic gradient over the free log-parameters of
            # (sigma2, phi_s, phi_t, tau2) (nngp_bf_grad_sep), the kinds fixed to the model's; fix_tau2, mean, X, tol
            # (L-BFGS-B's gtol), maxiter and reneighbor=r as for anisotropic=True.  gradient=False: Nelder-Mead on the
            # forward sweep (``gradient`` left at None means True here, False for every other model).
            for on, what in ((stderr, "stderr=True"), (method == "fisher", "method='fisher'"), (reml, "reml=True"),
                             (noise is not None, "noise="), (anisotropic, "anisotropic=True"),
                             (estimate_nu is not None, "estimate_nu"), (kind is not None, "kind="),
                             (nu is not None, "nu=")):
                if on:
                    _refuse_sep(self.cov, f"fit with {what}")
            if mean == "linear" and X is None:
                raise ValueError("mean='linear' needs the design matrix X")
            if mean != "linear" and X is not None:
                raise ValueError("X is the design of mean='linear'")
            return self._fit_sep(x0, mean, fix_tau2, method, maxiter, X, int(reneighbor), algo, tol,
                                 gradient_asked is None or gradient)
        if noise is not None:
            for on, what in ((stderr, "stderr=True"), (method == "fisher", "method='fisher'"),
                             (anisotropic, "anisotropic=True"), (estimate_nu is not None, "estimate_nu"),
                             (kind == "matern", "the general-nu matern kind"), (mean == "linear", "mean='linear'"),
                             (reml, "reml=True (a regression mean)")):
                if on:
                    _refuse_noise(f"fit with {what}")
        if estimate_nu is not None:
            for on, what in ((reml, "reml=True"), (anisotropic, "anisotropic=True"),
                             (method == "fisher", "method='fisher'"), (stderr, "stderr=True")):
                if on:
                    raise NotImplementedError(f"fit(estimate_nu=...) with {what}: the general-nu matern kind has a "
                                              "gradient sweep only (no restricted likelihood gradient, per-axis form "
                                              "or Fisher information sweep)")
        if mean == "linear" and X is None:
            raise ValueError("mean='linear' needs the design matrix X")
        if mean != "linear" and X is not None:
            raise ValueError("X is the design of mean='linear'")
        if estimate_nu is not None:
            return self._fit_matern(kind, x0, mean, fix_tau2, method or "L-BFGS-B", maxiter, X, algo, tol, nu,
                                    bool(estimate_nu), nu_bounds)
        if anisotropic:
            if stderr or method == "fisher":
                raise NotImplementedError("the Fisher information sweep has no per-axis form: fit(anisotropic=True) "
                                          "takes neither stderr=True nor method='fisher'")
            if reml:
                raise NotImplementedError("the restricted likelihood has no analytic gradient: anisotropic=True "
                                          "maximises the profile likelihood (reml=False)")
            if nu is not None:
                raise ValueError("nu is the smoothness of the general-nu matern kind, which anisotropic=True does not "
                                 "serve")
            return self._fit_aniso(kind, x0, mean, fix_tau2, method or "L-BFGS-B", maxiter, X, int(reneighbor), algo,
                                   tol)
        if reneighbor:
            raise ValueError("reneighbor is an option of anisotropic=True")
        _refuse_aniso(self.cov, "fit without anisotropic=True")
        if method == "fisher" or stderr:  # refused before any sweep, as gradient=True's kinds and m are
            if method == "fisher" and reml:
                raise NotImplementedError("the restricted likelihood has no analytic gradient or information: "
                                          "method='fisher' maximises the profile likelihood (reml=False)")
            if kind is None:
                self._grad_cov(None, aniso=False)
            elif kind == "matern":
                raise NotImplementedError("the analytic gradient does not serve the general-nu matern kind")
            elif not 1 <= self.m <= _lib.GRAD_MAX_M:
                raise NotImplementedError(f"the analytic gradient serves 1 <= m <= {_lib.GRAD_MAX_M} (m={self.m})")
        if reml:
            if gradient:
                raise NotImplementedError("the restricted likelihood has no analytic gradient: use gradient=False")
            if mean == "zero":
                raise ValueError("reml needs a mean to restrict by: mean='constant' or 'linear'")
            if mean == "constant":
                X = np.ones((self.nbr.shape[0], 1))
        linear = mean == "linear" or reml
        if linear:  # uploaded once: every evaluation below reuses the device tensor
            from . import regression

            X = regression.design(self, X, self.nbr.shape[0])

        if method is None:
            method = "L-BFGS-B" if gradient else "Nelder-Mead"

        base = self.cov if isinstance(self.cov, Covariance) else None
        kind = kind or (base.kind if base is not None else "exponential")
        if nu is None and base is not None and base.kind == kind:
            nu = base.nu
        th0 = tuple(x0) if x0 is not None else (base.theta[:3] if base is not None else (1.0, 10.0, 0.1))
        free_tau = fix_tau2 is None
        # noise=: resolved (and refused) once, before any sweep; every evaluation reuses the device weights
        nz = None if noise is None else _NoiseVar(self._noise_setup(noise, Covariance(kind, *th0, nu=nu))[1])
        if method == "fisher":
            return self._fit_fisher(kind, th0, nu, mean, X, linear, free_tau, fix_tau2, maxiter, tol, algo)
        from scipy.optimize import minimize

        def with_stderr(result):
            if stderr:
                result.update(self._fit_stderr(kind, result["theta"], nu, mean, X, free_tau))
            return result

        z0 = [math.log(th0[0]), math.log(th0[1])] + ([math.log(max(th0[2], 1e-6))] if free_tau else [])

        def theta_of(z):
            return (math.exp(z[0]), math.exp(z[1]), math.exp(z[2]) if free_tau else float(fix_tau2))

        best = {"ll": -math.inf}

        def obj(z):
            th = theta_of(z)
            try:
                if linear:
                    g = self.gls(Covariance(kind, *th, nu=nu), X, reml=reml, algo=algo)
                    ll, mu = g.objective, None
                else:
                    ll, mu = self.profile_loglik(Covariance(kind, *th, nu=nu), mean=mean, algo=algo, noise=nz)
            except NNGPNumericalError:
                return 1e300
            if ll > best["ll"]:
                best.update(ll=ll, mu=mu, theta=th)
            return -ll

        n_grad, last_failed = [0], [False]

        def obj_grad(z):
            th = theta_of(z)
            try:
                ll, mu, g = self.profile_loglik_grad(Covariance(kind, *th, nu=nu), mean=mean, X=X, noise=nz)
                mu = None if linear else mu
            except NNGPNumericalError:
                # no gradient exists here: the zero one can end a line search early, so the failure is kept
                # and shows in ``converged`` when the optimiser stops on such a point
                last_failed[0] = True
                return 1e300, np.zeros(len(z))
            last_failed[0] = False
            n_grad[0] += 1
            glog = np.array([th[k] * g[k] for k in range(len(z))])
            if ll > best["ll"]:
                best.update(ll=ll, mu=mu, theta=th, grad=glog)
            return -ll, -glog

        if gradient:
            self._grad_cov(Covariance(kind, *th0, nu=nu))  # refuse unsupported kinds / m before optimising
            opts = {"maxiter": maxiter}
            if nz is not None and tol is not None:
                opts.update(gtol=float(tol), ftol=1e-15)
            res = minimize(obj_grad, np.array(z0), jac=True, method=method, options=opts)
            self.cov = Covariance(kind, *best["theta"], nu=nu)
            self._B = self._F = None
            return with_stderr({"theta": best["theta"], "mu": best["mu"], "loglik": best["ll"],
                                "n_evals": int(res.nfev), "n_grad_evals": n_grad[0],
                                "converged": bool(res.success) and not last_failed[0],
                                **({} if nz is None else {"grad": best["grad"]}),
                                **self._fit_beta(X if linear else None, algo)})
        res = minimize(obj, np.array(z0), method=method, options={"maxiter": maxiter, "xatol": 1e-6,
                                                                  "fatol": 1e-9} if method == "Nelder-Mead"
                       else {"maxiter": maxiter})
        self.cov = Covariance(kind, *best["theta"], nu=nu)
        self._B = self._F = None
        return with_stderr({"theta": best["theta"], "mu": best["mu"], "loglik": best["ll"], "n_evals": int(res.nfev),
                            "converged": bool(res.success), **self._fit_beta(X if linear else None, algo)})

    def _fit_aniso(self, kind, x0, mean, fix_tau2, method, maxiter, X, reneighbor: int, algo: str, tol) -> dict:
        """``fit(anisotropic=True)``: gradient=True's scaffolding over (sigma2, phi_1 .. phi_dim, tau2)."""
        from scipy.optimize import minimize

        if reneighbor < 0:
            raise ValueError("reneighbor must be >= 0")
        dim = self._s_dev.shape[1]
        base = self.cov if isinstance(self.cov, (Covariance, AnisotropicCovariance)) else None
        kind = kind or (base.kind if base is not None else "exponential")
        if x0 is not None:
            if len(x0) != 3:
                raise ValueError("x0 must be (sigma2, phi, tau2) with phi one number or one per axis")
            s0, p0, t0 = x0
        elif base is not None:
            s0, p0, t0 = base.sigma2, base.phi, base.tau2
        else:
            s0, p0, t0 = 1.0, 10.0, 0.1
        p0 = tuple(float(p) for p in p0) if np.ndim(p0) else (float(p0),) * dim
        free_tau = fix_tau2 is None
        linear = mean == "linear"
        if linear:
            from . import regression

            X = regression.design(self, X, self.nbr.shape[0])

        def cov_of(z):
            return AnisotropicCovariance(kind, math.exp(z[0]), tuple(math.exp(v) for v in z[1:1 + dim]),
                                         math.exp(z[1 + dim]) if free_tau else float(fix_tau2))

        start = AnisotropicCovariance(kind, float(s0), p0, max(float(t0), 1e-6) if free_tau else float(fix_tau2))
        self._grad_cov(start)  # refuse a wrong len(phi) or an unsupported m before optimising
        n_evals = n_grad = 0
        options, kw = {"maxiter": maxiter}, {}
        if tol is not None and method == "L-BFGS-B":
            options["gtol"] = float(tol)  # the gradient rule alone; scipy's tol= would set ftol to it as well
        elif tol is not None:
            kw["tol"] = float(tol)
        for rnd in range(reneighbor + 1):
            if rnd > 0:
                self.rebuild_neighbors(start)
            best, seen, last_failed = {"ll": -math.inf}, {}, [False]

            def obj_grad(z):
                cv = cov_of(z)
                try:
                    ll, mu, g = self.profile_loglik_grad(cv, mean=mean, X=X)
                except NNGPNumericalError:
                    last_failed[0] = True
                    return 1e300, np.zeros(len(z))
                last_failed[0] = False
                th = cv.theta
                gz = np.array([th[k] * g[k] for k in range(len(z))])
                seen[tuple(z)] = gz
                if ll > best["ll"]:
                    best.update(ll=ll, mu=None if linear else mu, cov=cv)
                return -ll, -gz

            th = start.theta
            z0 = np.log(np.array(th[:1 + dim + (1 if free_tau else 0)]))
            res = minimize(obj_grad, z0, jac=True, method=method, options=options, **kw)
            n_evals += int(res.nfev)
            n_grad += len(seen)
            if "cov" not in best:
                raise NNGPNumericalError("fit(anisotropic=True): no parameter value the optimiser tried was positive "
                                         "definite")
            start = best["cov"]
        self.cov = start
        self._B = self._F = None
        if reneighbor > 0:
            # leave the sets in the estimate's own metric and report the likelihood on them (grad stays the last
            # round's: the gradient on the sets that round optimised over)
            self.rebuild_neighbors(start)
            if linear:
                best["ll"] = self.gls(start, X, algo=algo).loglik
            else:
                best["ll"], best["mu"] = self.profile_loglik(start, mean=mean, algo=algo)
        return {"theta": start.theta, "sigma2": start.sigma2, "phi": start.phi, "tau2": start.tau2, "mu": best["mu"],
                "loglik": best["ll"], "grad": -np.asarray(res.jac, dtype=np.float64), "n_evals": n_evals,
                "n_grad_evals": n_grad, "converged": bool(res.success) and not last_failed[0],
                "message": str(res.message), "rounds": reneighbor + 1,
                **self._fit_beta(X if linear else None, algo)}

    def _fit_sep(self, x0, mean, fix_tau2, method, maxiter, X, reneighbor: int, algo: str, tol, gradient: bool) -> dict:
        """``fit`` of a :class:`SeparableCovariance` model: _fit_aniso's scaffolding over (sigma2, phi_s, phi_t,
        tau2), or Nelder-Mead on the forward sweep (``gradient`` False)."""
        from scipy.optimize import minimize

        if reneighbor < 0:
            raise ValueError("reneighbor must be >= 0")
        base = self._sep_model(self.cov)
        if x0 is not None and len(x0) != 4:
            raise ValueError("x0 must be (sigma2, phi_s, phi_t, tau2)")
        s0, ps0, pt0, t0 = (float(v) for v in (x0 if x0 is not None else base.theta))
        free_tau = fix_tau2 is None
        linear = mean == "linear"
        if mean not in ("constant", "zero", "linear"):
            raise ValueError("mean must be 'constant', 'zero' or 'linear'")
        if linear:
            from . import regression

            X = regression.design(self, X, self.nbr.shape[0])
        if method is None:
            method = "L-BFGS-B" if gradient else "Nelder-Mead"
        nz = 3 + (1 if free_tau else 0)

        def cov_of(z):
            return SeparableCovariance(base.kind_s, base.kind_t, math.exp(z[0]), math.exp(z[1]), math.exp(z[2]),
                                       math.exp(z[3]) if free_tau else float(fix_tau2))

        start = SeparableCovariance(base.kind_s, base.kind_t, s0, ps0, pt0,
                                    max(t0, 1e-6) if free_tau else float(fix_tau2))
        n_evals = n_grad = 0
        if gradient:
            options = {"maxiter": maxiter}
            if tol is not None and method == "L-BFGS-B":
                options.update(gtol=float(tol), ftol=1e-15)  # the gradient rule alone
            elif tol is not None:
                options["gtol"] = float(tol)
        else:
            options = {"maxiter": maxiter}
            if method == "Nelder-Mead":
                options.update(xatol=1e-6 if tol is None else float(tol), fatol=1e-9)
        for rnd in range(reneighbor + 1):
            if rnd > 0:
                self.rebuild_neighbors(start)
            best, seen, last_failed = {"ll": -math.inf}, {}, [False]

            def cov_at(z):
                """The covariance at log-parameters z, or None where exp(z) leaves the positive finite doubles (a line
                search's far step): both objectives then return the penalty value."""
                try:
                    return cov_of(z)
                except (OverflowError, ValueError):
                    return None

            def obj_grad(z):
                cv = cov_at(z)
                try:
                    if cv is None:
                        raise NNGPNumericalError("theta outside the positive finite doubles")
                    ll, mu, g = self.profile_loglik_grad(cv, mean=mean, X=X)
                except NNGPIndexError:  # a bad neighbour index is no property of theta
                    raise
                except NNGPNumericalError:
                    last_failed[0] = True
                    return 1e300, np.zeros(len(z))
                last_failed[0] = False
                th = cv.theta
                gz = np.array([th[k] * g[k] for k in range(len(z))])
                seen[tuple(z)] = gz
                if ll > best["ll"]:
                    best.update(ll=ll, mu=None if linear else mu, cov=cv, grad=gz)
                return -ll, -gz

            def obj(z):
                cv = cov_at(z)
                try:
                    if cv is None:
                        raise NNGPNumericalError("theta outside the positive finite doubles")
                    ll, mu = self.profile_loglik(cv, mean=mean, X=X)
                except NNGPIndexError:
                    raise
                except NNGPNumericalError:
                    return 1e300
                if ll > best["ll"]:
                    best.update(ll=ll, mu=None if linear else mu, cov=cv)
                return -ll

            z0 = np.log(np.array(start.theta[:nz]))
            if gradient:
                res = minimize(obj_grad, z0, jac=True, method=method, options=options)
            else:
                res = minimize(obj, z0, method=method, options=options)
            n_evals += int(res.nfev)
            n_grad += len(seen)
            if "cov" not in best:
                raise NNGPNumericalError("fit (SeparableCovariance): no parameter value the optimiser tried was "
                                         "positive definite")
            start = best["cov"]
        self.cov = start
        self._B = self._F = None
        if reneighbor > 0:
            # as fit(anisotropic=True): the sets in the estimate's own metric, the likelihood on them
            self.rebuild_neighbors(start)
            if linear:
                best["ll"] = self.gls(start, X, algo=algo).loglik
            else:
                best["ll"], best["mu"] = self.profile_loglik(start, mean=mean, algo=algo)
        out = {"theta": start.theta, "sigma2": start.sigma2, "phi_s": start.phi_s, "phi_t": start.phi_t,
               "tau2": start.tau2, "mu": best["mu"], "loglik": best["ll"], "n_evals": n_evals, "n_grad_evals": n_grad,
               "converged": bool(res.success) and not last_failed[0], "message": str(res.message),
               "rounds": reneighbor + 1, **self._fit_beta(X if linear else None, algo)}
        if gradient:
            out["grad"] = best["grad"]  # at the reported theta (the best point seen, the last round's)
        return out

    def _fit_matern(self, kind, x0, mean, fix_tau2, method, maxiter, X, algo, tol, nu, free_nu: bool,
                    nu_bounds) -> dict:
        """``fit(estimate_nu=...)``: gradient=True's scaffolding over (sigma2, phi, tau2[, nu])."""
        from scipy.optimize import minimize

        _refuse_aniso(self.cov, "fit(estimate_nu=...)")
        base = self.cov if isinstance(self.cov, Covariance) else None
        kind = kind or (base.kind if base is not None else None)
        if kind != "matern":
            raise ValueError(f"estimate_nu is an option of kind='matern' (kind={kind!r})")
        if nu is None and base is not None and base.kind == "matern":
            nu = base.nu
        lo, hi = (float(b) for b in nu_bounds)
        if not 0.0 < lo < hi <= _lib.MATERN_NU_MAX:
            raise ValueError(f"nu_bounds must satisfy 0 < lo < hi <= {_lib.MATERN_NU_MAX:g}")
        th0 = tuple(x0)[:3] if x0 is not None else (base.theta[:3] if base is not None else (1.0, 10.0, 0.1))
        free_tau = fix_tau2 is None
        linear = mean == "linear"
        if linear:
            from . import regression

            X = regression.design(self, X, self.nbr.shape[0])
        start = MaternCovariance(float(th0[0]), float(th0[1]),
                                 max(float(th0[2]), 1e-6) if free_tau else float(fix_tau2),
                                 min(max(float(nu), lo), hi) if free_nu and nu is not None else nu)
        self._grad_cov(start)  # refuse an unsupported m before optimising
        idx = [0, 1] + ([2] if free_tau else []) + ([3] if free_nu else [])  # theta's free entries

        def cov_of(z):
            th = list(start.theta)
            for k, j in enumerate(idx):
                th[j] = math.exp(z[k])
            return MaternCovariance(*th)

        best, last_failed, n_grad = {"ll": -math.inf}, [False], [0]

        def obj_grad(z):
            cv = cov_of(z)
            try:
                ll, mu, g = self.profile_loglik_grad(cv, mean=mean, X=X)
            except NNGPNumericalError:
                last_failed[0] = True
                return 1e300, np.zeros(len(z))
            last_failed[0] = False
            n_grad[0] += 1
            th = cv.theta
            if ll > best["ll"]:
                best.update(ll=ll, mu=None if linear else mu, cov=cv)
            return -ll, -np.array([th[j] * g[j] for j in idx])

        options, kw = {"maxiter": maxiter}, {}
        if tol is not None and method == "L-BFGS-B":
            # the gradient rule alone decides: the relative-decrease rule (ftol) is set below any step it could end,
            # so a converged fit reports a gradient within tol
            options["gtol"] = float(tol)
            options["ftol"] = 1e-15
        elif tol is not None:
            kw["tol"] = float(tol)
        if method == "L-BFGS-B":
            kw["bounds"] = [(math.log(lo), math.log(hi)) if j == 3 else (None, None) for j in idx]
        z0 = np.log(np.array([start.theta[j] for j in idx]))
        res = minimize(obj_grad, z0, jac=True, method=method, options=options, **kw)
        if "cov" not in best:
            raise NNGPNumericalError("fit(estimate_nu=...): no parameter value the optimiser tried was positive "
                                     "definite")
        cv = best["cov"]
        self.cov = cv
        self._B = self._F = None
        return {"theta": cv.theta, "sigma2": cv.sigma2, "phi": cv.phi, "tau2": cv.tau2, "nu": float(cv.nu),
                "mu": best["mu"], "loglik": best["ll"], "grad": -np.asarray(res.jac, dtype=np.float64),
                "n_evals": int(res.nfev), "n_grad_evals": n_grad[0],
                "converged": bool(res.success) and not last_failed[0], "message": str(res.message),
                **self._fit_beta(X if linear else None, algo)}

    def _fit_beta(self, X, algo):
        """``beta`` and ``cov_beta`` of a regression fit at the estimate ``self.cov`` (nothing without a design)."""
        if X is None:
            return {}
        g = self.gls(self.cov, X, algo=algo)
        return {"beta": g.beta, "cov_beta": g.cov_beta}

    # -- latent field at fixed theta --------------------------------------------
    def _latent_posterior(self, cov, mean: str):
        """The :class:`pynngp_amd.LatentPosterior` of this instance's ``y`` / ``eps`` / neighbour sets at ``cov``
        (kept between calls; a new theta of the same mean is one ``update``)."""
        _refuse_aniso(self.cov if cov is None else cov, "the latent posterior")
        if not self._same_sets():
            raise NotImplementedError("the latent posterior serves refType == 'S=T' (the field on the data "
                                      f"locations), not {self.refType!r}")
        if mean not in ("constant", "zero"):
            raise ValueError("mean must be 'constant' or 'zero'")
        from .latent import LatentPosterior

        cv = self.cov if cov is None else cov
        held = getattr(self, "_latent", None)
        if held is not None and held[0] == mean and held[1] is self.nbr:
            if held[2].cov != cv:
                held[2].update(cv)
            return held[2]
        y = np.asarray(self.y, dtype=np.float64)
        eps = None
        if self.eps is not None:  # per-location measurement sigmas (nngp.py:9), as oneSample takes them
            ev = np.asarray(self.eps, dtype=np.float64)
            if ev.shape == y.shape and np.all(np.isfinite(ev)) and np.all(ev > 0):
                eps = ev
        X = np.ones((y.shape[0], 1)) if mean == "constant" and y.ndim == 1 else None
        lp = LatentPosterior(self.t, y, cv, m=self.m, X=X, eps=eps, device=self.device, nbr=self.nbr)
        self._latent = (mean, self.nbr, lp)
        return lp

    def latent_posterior(self, cov: Optional[Covariance] = None, mean: str = "constant"):
        """The :class:`pynngp_amd.LatentPosterior` of this instance at ``cov`` (default ``self.cov``), for every
        ``refType``: 'S=T' puts the field on the data locations (and reuses the neighbour sets held here); a
        tuple refType puts it on ``s`` with the data locations outside S as leaves that are integrated out
        (``LatentPosterior(ref=s)``), so the solver's vectors have one entry per reference point.  Kept between
        calls: a new theta of the same mean is one ``update``.  ``mean="constant"`` estimates an intercept by GLS,
        ``"zero"`` takes y as centred; NaN in ``y`` = unobserved; ``eps`` as :meth:`latent_mean`.  Its ``mean`` /
        ``sample`` / ``marginal_variance`` take ``where="data"`` or ``"ref"``, and ``predict(query)`` gives the
        mean, variance and draws at new locations."""
        _refuse_aniso(self.cov if cov is None else cov, "the latent posterior")
        if self._same_sets():
            return self._latent_posterior(cov, mean)
        if mean not in ("constant", "zero"):
            raise ValueError("mean must be 'constant' or 'zero'")
        from .latent import LatentPosterior

        cv = self.cov if cov is None else cov
        held = getattr(self, "_latent_ref", None)
        if held is not None and held[0] == mean and held[1] is self.s:
            if held[2].cov != cv:
                held[2].update(cv)
            return held[2]
        y = np.asarray(self.y, dtype=np.float64)
        eps = None
        if self.eps is not None:
            ev = np.asarray(self.eps, dtype=np.float64)
            if ev.shape == y.shape and np.all(np.isfinite(ev)) and np.all(ev > 0):
                eps = ev
        X = np.ones((y.shape[0], 1)) if mean == "constant" and y.ndim == 1 else None
        lp = LatentPosterior(self.t, y, cv, m=self.m, X=X, eps=eps, device=self.device, ref=self.s)
        self._latent_ref = (mean, self.s, lp)
        return lp

    def latent_loglik(self, cov: Optional[Covariance] = None, mean: str = "constant", **kw):
        """``(value, se)``: log p(y | theta) of the LATENT model y = mu + w + e, w the NNGP on S, at ``cov`` (default
        ``self.cov``), for every ``refType`` -- :meth:`pynngp_amd.LatentPosterior.log_marginal` of
        :meth:`latent_posterior`, which takes ``**kw`` (``n_probes``, ``seed``, ``rtol``, ...).  ``se`` is the
        standard error of the stochastic log-determinant term.  Not :meth:`loglik`, which puts the NNGP on y itself
        and serves S = T only.  ``mean="constant"`` plugs in the GLS intercept (a profiled likelihood)."""
        return self.latent_posterior(cov, mean).log_marginal(**kw)

    def latent_loglik_grad(self, cov: Optional[Covariance] = None, mean: str = "constant", **kw):
        """``(value, se, grad, grad_se)``: :meth:`latent_loglik` with its gradient in (sigma2, phi, tau2) and the
        gradient's standard errors -- :meth:`pynngp_amd.LatentPosterior.log_marginal_grad` of
        :meth:`latent_posterior` (``**kw`` as there).  The fused kinds exponential .. spherical, m <= 32."""
        return self.latent_posterior(cov, mean).log_marginal_grad(**kw)

    def latent_fit(self, mean: str = "constant", **kw):
        """Empirical-Bayes (sigma2, phi, tau2) of the latent model, for every ``refType``:
        :meth:`pynngp_amd.LatentPosterior.fit` (derivative-free by default, ``gradient=True``: L-BFGS-B on the
        analytic gradient; common random numbers; ``**kw`` as there: ``x0``, ``fix_tau2``, ``n_probes``, ``seed``,
        ``method``, ``maxiter``, ``gradient``) from ``self.cov``.  Sets ``cov`` to the estimate and returns ``(cov,
        result)``."""
        cov, res = self.latent_posterior(None, mean).fit(**kw)
        self.cov = cov
        self._B = self._F = None
        return cov, res

    def latent_mean(self, cov: Optional[Covariance] = None, rtol: float = 1e-8, mean: str = "constant"):
        """Posterior mean of the latent field w on the data locations at a fixed ``cov`` (default ``self.cov``,
        e.g. after :meth:`fit`): ``(w_hat, beta_hat)`` from a conjugate-gradient solve with the NNGP posterior
        precision (:class:`pynngp_amd.LatentPosterior`) -- the deterministic estimator of the reference's ``ws`` /
        ``wt`` state (nngp.py:42-47).  ``mean="constant"`` estimates an intercept by GLS (as :meth:`fit`
        profiles it out), ``"zero"`` takes y as centred.  NaN in ``y`` = unobserved; ``eps``, when it is one
        positive sigma per location, scales the noise variance to tau2 eps_i^2.  refType 'S=T' only; for a
        reference set (and for prediction with uncertainty) use :meth:`latent_posterior`.
        The latent mean at new locations is ``predict(values=w_hat, cov=cov.replace(tau2=0), query=...)``."""
        return self._latent_posterior(cov, mean).mean(rtol=rtol)

    def latent_sample(self, n: int, cov: Optional[Covariance] = None, seed: int = 0, mean: str = "constant"):
        """``(n, N)`` exact draws of w | y, theta at a fixed ``cov`` (perturbation sampling on the same solver;
        Philox normals keyed by ``seed``).  refType 'S=T' only (a reference set: :meth:`latent_posterior`);
        arguments as :meth:`latent_mean`."""
        return self._latent_posterior(cov, mean).sample(n, seed=seed)

    def latent_sd(self, n_draws: int = 64, cov: Optional[Covariance] = None, seed: int = 0,
                  mean: str = "constant") -> np.ndarray:
        """``(N,)`` posterior standard deviations of w | y, theta at a fixed ``cov``: the square root of
        :meth:`pynngp_amd.LatentPosterior.marginal_variance` (Rao-Blackwellised over ``n_draws`` exact draws,
        relative standard error about sqrt(2 / (n_draws - 1)) at worst).  refType 'S=T' only (a reference set:
        :meth:`latent_posterior`); arguments as :meth:`latent_mean`."""
        return np.sqrt(self._latent_posterior(cov, mean).marginal_variance(n_draws, seed=seed))

    # -- simulation from the prior ------------------------------------------------
    NOISE_STREAM = 1 << 41  # Philox sweep index of simulate's noise for draw k: NOISE_STREAM + k (no draw's stream)

    def prior_factor(self, cov: Optional[Covariance] = None):
        """The :class:`pynngp_amd.NNGPFactor` of this instance at ``cov`` (default ``self.cov``): the factor of the
        NNGP prior on ``s`` with the data locations outside it as leaves, for triangular solves, covariance
        products and prior draws.  'S=T' reuses the neighbour sets held here.  Kept between calls: a new theta is
        one ``update``."""
        from .factor import NNGPFactor, _check_cov

        _refuse_aniso(self.cov if cov is None else cov, "the prior factor (prior_factor, simulate)")
        cv = _check_cov(self.cov if cov is None else cov)
        held = getattr(self, "_factor", None)
        key = self.nbr if self._same_sets() else self.s
        if held is not None and held[0] is key:
            if held[1].cov != cv:
                held[1].update(cv)
            return held[1]
        if self._same_sets():
            f = NNGPFactor(self.t, cv, m=self.m, nbr=self.nbr, device=self.device)
        else:
            f = NNGPFactor(self.t, cv, m=self.m, device=self.device, ref=self.s)
        self._factor = (key, f)
        return f

    def simulate(self, n_draws: int = 1, seed: int = 0, cov: Optional[Covariance] = None, beta=None, X=None,
                 noise: bool = True) -> np.ndarray:
        """``(n_draws, N)`` simulated responses y = X beta + w + e on this instance's own locations ``t``: w a draw
        from the NNGP prior at ``cov`` (default ``self.cov``) by :meth:`pynngp_amd.NNGPFactor.sample_prior` -- a
        level-scheduled triangular solve, no dense Cholesky, so it serves the sizes the sweeps serve -- and
        e_i ~ N(0, tau2 eps_i^2) (``eps`` when it is one positive sigma per location, else 1; ``noise=False`` or
        tau2 = 0: none).  ``X`` (N, p) with ``beta`` (p,), or a scalar ``beta`` as the constant mean; default 0.
        Philox normals keyed by ``seed``: one seed repeats bit for bit, and draw k does not depend on ``n_draws``."""
        f = self.prior_factor(cov)
        n_draws = int(n_draws)
        W = f._draws(n_draws, seed, None)[f._node_of_t_dev]  # (N, n_draws) on the device
        n = W.shape[0]
        if noise and f.cov.tau2 > 0:
            sd = torch.full((n,), math.sqrt(f.cov.tau2), dtype=torch.float64, device=self.device)
            if self.eps is not None:
                ev = np.asarray(self.eps, dtype=np.float64)
                if ev.shape == (n,) and np.all(np.isfinite(ev)) and np.all(ev > 0):
                    sd = sd * torch.from_numpy(ev).to(self.device)
            z = torch.empty(n, dtype=torch.float64, device=self.device)
            for k in range(n_draws):
                W[:, k] += sd * _lib.gibbs_normals(z, seed, self.NOISE_STREAM + k)
        out = W.t().cpu().numpy()
        if beta is not None:
            bv = np.asarray(beta, dtype=np.float64)
            if X is None:
                if bv.ndim != 0:
                    raise ValueError("beta without X must be a scalar (the constant mean)")
                out = out + float(bv)
            else:
                Xh = np.asarray(X, dtype=np.float64)
                Xh = Xh[:, None] if Xh.ndim == 1 else Xh
                if Xh.shape[0] != n or bv.reshape(-1).shape != (Xh.shape[1],):
                    raise ValueError(f"X must be ({n}, p) and beta (p,), got {Xh.shape} and {bv.shape}")
                out = out + (Xh @ bv.reshape(-1))[None, :]
        elif X is not None:
            raise ValueError("X needs beta")
        return out

    def oneSample(self, seed: int = 0, X=None, **sampler_kw):
        """One Gibbs iteration of the response model y = X beta + w + eps: the reference's
        ``update_wt`` / ``update_ws`` / ``update_y_unobserved`` (nngp.py:98-101, which do not
        exist there), delegated to :class:`pynngp_amd.SeqNNGP`, created on the first call
        with (sigma2, phi, tau2) from ``cov`` and w initialised from ``ws`` (reference
        points) and ``wt`` (data locations outside S; NaN -> 0).  'S=T': the field lives on
        the data locations; tuple refTypes: on S, with each data location outside S a leaf
        linked to its ``Nt`` (nngp.py:64-71).  ``X`` defaults to an intercept (pass
        ``X_ref`` for the covariates at S to get predictive draws there).  ``eps``
        (nngp.py:9, "measurement uncertainties in y"), when it is one positive sigma per
        location, makes the noise heteroscedastic: variance tau2 eps_i^2 (see SeqNNGP;
        ``fix_tau2=True`` with tau2 = 1 for exactly eps_i^2).  Afterwards ``ws`` / ``wt``
        hold the current w at S / T and ``y_unobserved`` the current predictive draws.
        Returns the sampler (its ``beta, sigma2, tau2, phi`` are the other draws).  With the
        reference's plug-in ``cov(a, b)`` (a callable) the covariance is held fixed: its blocks are
        evaluated once, and w, tau2 and beta are sampled (no phi / sigma2: the callable has no such
        parameters; its nugget ``CallableCovariance(fn, tau2)`` starts tau2)."""
        y = np.asarray(self.y, dtype=np.float64)
        if y.ndim != 1:
            raise ValueError("oneSample needs one response per location (1-D y)")
        _refuse_aniso(self.cov, "the Gibbs sampler (oneSample)")
        if getattr(self, "_sampler", None) is None:
            from .gibbs import SeqNNGP

            cv = self._covariance()
            if isinstance(cv, IsotropicCovariance):
                raise TypeError("the Gibbs sampler takes a built-in covariance kind (pynngp_amd.Covariance) or the "
                                "reference's plug-in cov(a, b) (a callable / CallableCovariance), not an "
                                "IsotropicCovariance: write it as cov(a, b)")
            if "eps" not in sampler_kw and self.eps is not None:
                ev = np.asarray(self.eps, dtype=np.float64)
                if ev.shape == y.shape and np.all(np.isfinite(ev)) and np.all(ev > 0):
                    sampler_kw["eps"] = ev
            ref = None if self._same_sets() else self.s
            if isinstance(cv, CallableCovariance):
                # the plug-in held fixed: w, tau2, beta sampled; no phi / sigma2 (the callable carries its own
                # scale); the nugget, when given, starts tau2
                tau2 = cv.tau2 if cv.tau2 > 0 else 0.1
                smp = SeqNNGP(self.t, y, X=X, m=self.m, cov=cv, tau2=tau2, seed=seed, device=self.device, ref=ref,
                              **sampler_kw)
            else:
                tau2 = cv.tau2 if cv.tau2 > 0 else 0.1 * cv.sigma2
                smp = SeqNNGP(self.t, y, X=X, m=self.m, kind=cv.kind, sigma2=cv.sigma2, tau2=tau2, phi=cv.phi,
                              seed=seed, device=self.device, ref=ref, nu=cv.nu_arg, **sampler_kw)
            ws = np.asarray(self.ws, dtype=np.float64)
            smp.set_w(ws=np.where(np.isfinite(ws), ws, 0.0),
                      wt=None if ref is None else np.where(np.isfinite(self.wt), self.wt, 0.0))
            self._sampler = smp
        self._sampler.step()
        self.ws = self._sampler.w_s.cpu().numpy()
        self.wt = self._sampler.w_t.cpu().numpy()
        self.y_unobserved = self._sampler.y_unobserved.cpu().numpy()
        return self._sampler


def reference_set(t, refType, device=None):
    """S for a refType (nngp.py:21-40).  The tuple forms draw from numpy's global RNG with
    the reference's own calls: ('subset', nRef) -> t[np.random.choice(len(t), size=nRef)]
    (with replacement, as nngp.py:36); ('random', nRef, bounds) -> one
    np.random.uniform(lo, hi, nRef) column per (lo, hi) in bounds (nngp.py:39-40).
    ('maxmin', nRef) -> the first nRef points of the max-min order of t, in that order (no RNG; distinct,
    space-filling; computed on ``device``, default the current GPU)."""
    if isinstance(refType, str):
        if refType != "S=T":
            raise ValueError(f"unknown refType {refType!r} (only 'S=T' is a string option)")
        return t
    if isinstance(refType, tuple) and len(refType) >= 2:
        typ = refType[0]
        if typ == "subset":
            choice = np.random.choice(len(t), size=int(refType[1]))
            return np.asarray(t)[choice]
        if typ == "random":
            if len(refType) < 3:
                raise ValueError("('random', nRef, bounds) needs bounds")
            nRef, bounds = int(refType[1]), refType[2]
            return np.vstack([np.random.uniform(lo, hi, nRef) for lo, hi in bounds]).T
        if typ == "maxmin":
            from .ordering import maxmin_subset

            t_host = np.ascontiguousarray(t, dtype=np.float64)
            pts = torch.as_tensor(t_host[:, None] if t_host.ndim == 1 else t_host).to(_default_device(device))
            return np.asarray(t)[maxmin_subset(pts, int(refType[1])).cpu().numpy()]
        raise ValueError(f"unknown refType kind {typ!r} (expected 'subset', 'random' or 'maxmin')")
    raise TypeError(f"refType must be 'S=T' or a tuple, got {refType!r}")


class NNGPNumericalError(ArithmeticError):
    """A location's neighbour covariance was not positive definite."""


class NNGPIndexError(NNGPNumericalError, IndexError):
    """A neighbour index was out of range, as a :class:`SeparableCovariance` model reports it: both of the sweep's
    flags surface as :class:`NNGPNumericalError` there (it is an ``IndexError`` too, what every other model raises)."""


def _raise_on_bad(partials_host, cov=None) -> None:
    if partials_host[3] >= 0 and isinstance(cov, SeparableCovariance):
        raise NNGPIndexError(f"neighbour index out of range at location {int(partials_host[3])}")
    if partials_host[3] >= 0:
        raise IndexError(f"neighbour index out of range at location {int(partials_host[3])}")
    if partials_host[2] >= 0:
        raise NNGPNumericalError(
            f"non-positive Cholesky pivot or F at location {int(partials_host[2])} (add a nugget tau2 or change phi)")
