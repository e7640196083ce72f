"""Point orderings for the Vecchia / NNGP factorisation: which point conditions on which.

A Vecchia approximation conditions every point on its ``m`` nearest *earlier* points, so its quality depends on
the order as much as on ``m``.  The functions here return permutations (device int64 tensors, ``perm[k]`` = the
input row at position ``k``); ``NNGP(..., ordering=)`` applies one before it builds the neighbour sets.

* :func:`order_maxmin` -- the levelled max-min (nested-net) order, ``nngp_order_maxmin`` on the GPU (DESIGN.md
  4.4a): every point is far from all of its predecessors, so early points spread over the whole domain and later
  ones fill in.  Within a factor of 4 of the exact greedy max-min distance at every position outside the tail,
  fully parallel, and the same bits on every run.  Its first ``k`` points are a space-filling subset
  (:func:`maxmin_subset`).
* :func:`order_random` -- the same key sort without geometry.
* :func:`order_coordinate`, :func:`order_middleout` -- stable sorts by one coordinate / by the distance from the
  mean location, for comparison.

No order wins everywhere: in the measurements of DESIGN.md 4.4a max-min had the smallest KL divergence from the
exact process for exponential covariances with a nugget, while a Matern-3/2 field without a nugget was closer in
coordinate order.  A max-min order does not shorten the level schedule of the factor solves relative to a random
order; what a coordinate-sorted input needs there is any reordering.

There is no CPU fallback: CPU tensors raise, as everywhere in this package.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

ORDERINGS = ("maxmin", "random")


def _finite_coords(coords: torch.Tensor) -> torch.Tensor:
    if not torch.is_tensor(coords):
        raise TypeError("coords must be a torch tensor on a ROCm GPU")
    coords = _lib._as_coords(coords)
    if coords.shape[0] < 1:
        raise ValueError("an ordering needs at least one point")
    if not bool(torch.isfinite(coords).all()):
        raise ValueError("coords contain NaN or infinity")
    return coords


def order_maxmin(coords: torch.Tensor, seed: int = 0, return_level: bool = False):
    """Levelled max-min order of ``coords`` (float64 (n, d) device tensor, d <= 3): ``perm`` int64 (n,), and with
    ``return_level`` also ``level`` int32 (n,), the level of the point at each position (0 for the first point,
    1 .. 19, 20 for the tail of coincident and nearly coincident points).  ``seed`` (uint32) picks the keys that
    break ties inside a level.  A setup call: it synchronises the current stream once per round."""
    coords = _finite_coords(coords)
    perm, level = _lib.order_maxmin(coords, seed)
    return (perm, level) if return_level else perm


def _hashes(n: int, seed: int, device) -> torch.Tensor:
    """mix32((i + seed * 0x9e3779b9) mod 2^32), the murmur3 finaliser, as non-negative int64."""
    m = 0xFFFFFFFF
    h = (torch.arange(n, dtype=torch.int64, device=device) + ((int(seed) * 0x9E3779B9) & m)) & m
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & m
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & m
    return h ^ (h >> 16)


def order_random(n: int, seed: int = 0, device=None) -> torch.Tensor:
    """``argsort(key)`` for the keys of :func:`order_maxmin` (``mix32(i + seed * 0x9e3779b9) << 32 | i``): the
    same pseudo-random order on every run and machine."""
    if n < 1:
        raise ValueError("an ordering needs at least one point")
    if not 0 <= int(seed) < 2 ** 32:
        raise ValueError(f"seed must be a uint32, got {seed}")
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.NNGPExtensionError("pynngp_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is "
                                          "no CPU fallback")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.NNGPExtensionError(f"pynngp_amd needs a ROCm GPU device (got {device}); there is no CPU fallback")
    # a stable sort of the hashes from index order: ties fall to the smaller index, as the key's low word says
    return torch.sort(_hashes(int(n), seed, device), stable=True).indices


def order_coordinate(coords: torch.Tensor, axis: int = 0) -> torch.Tensor:
    """Stable sort by coordinate ``axis`` (ties keep the input order)."""
    coords = _finite_coords(coords)
    _lib._require_gpu(coords)
    if not 0 <= int(axis) < coords.shape[1]:
        raise ValueError(f"axis={axis} outside [0, {coords.shape[1]})")
    return torch.sort(coords[:, int(axis)], stable=True).indices


def order_middleout(coords: torch.Tensor) -> torch.Tensor:
    """Stable sort by the distance from the mean location, nearest first."""
    coords = _finite_coords(coords)
    _lib._require_gpu(coords)
    d2 = ((coords - coords.mean(dim=0, keepdim=True)) ** 2).sum(dim=1)
    return torch.sort(d2, stable=True).indices


def maxmin_subset(coords: torch.Tensor, k: int, seed: int = 0) -> torch.Tensor:
    """The first ``k`` rows of the max-min order: ``k`` distinct, space-filling points (int64 row indices)."""
    if not 1 <= int(k) <= coords.shape[0]:
        raise ValueError(f"k={k} outside [1, {coords.shape[0]}]")
    return order_maxmin(coords, seed)[: int(k)]


def check_permutation(perm, n: int) -> np.ndarray:
    """``perm`` as a host int64 array, checked to be a permutation of ``range(n)``."""
    p = perm.detach().cpu().numpy() if torch.is_tensor(perm) else np.asarray(perm)
    if p.ndim != 1 or p.shape[0] != n:
        raise ValueError(f"an explicit ordering must be a permutation of length {n}, got shape {tuple(p.shape)}")
    if not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"an explicit ordering must hold integers, got {p.dtype}")
    p = p.astype(np.int64)
    seen = np.zeros(n, dtype=bool)
    inside = (p >= 0) & (p < n)
    seen[p[inside]] = True
    if not inside.all() or not seen.all():
        raise ValueError(f"an explicit ordering must be a permutation of range({n})")
    return p


def resolve(ordering, coords: torch.Tensor) -> np.ndarray:
    """The permutation (host int64) that ``ordering`` -- "maxmin", "random" or an explicit permutation -- gives
    for the device points ``coords``."""
    n = coords.shape[0]
    if isinstance(ordering, str):
        if ordering == "maxmin":
            return order_maxmin(coords).cpu().numpy()
        if ordering == "random":
            return order_random(n, 0, coords.device).cpu().numpy()
        raise ValueError(f"unknown ordering {ordering!r} (expected one of {ORDERINGS}, a permutation or None)")
    return check_permutation(ordering, n)
