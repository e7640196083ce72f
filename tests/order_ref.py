"""Numpy restatement of the levelled max-min order (nngp_order_maxmin), shared by
test_order_host.py and test_gpu_order.py, with the exact greedy max-min order it approximates and the checks of
its defining properties.  Independent of the HIP code: the winners of a round are visited one after the other,
as the definition says, where the kernels run Luby rounds.

The definition.  dist2(a, b) = ((d0 d0) + (d1 d1)) + (d2 d2), every operation rounded on its own (numpy's
elementwise arithmetic does that).  key(i) = mix32((i + seed 0x9e3779b9) mod 2^32) << 32 | i; the smaller key
wins.  p1 = argmin dist2(x_i, c), c = 0.5 (lo + hi) the centre of the bounding box, ties to the smallest i;
R = sqrt(max dist2(x_i, p1)).  Level l = 1 .. 19: r = R 2^-l, r2 = r r, cells of side h = r c_d (c_1, c_2,
c_3 = 0.5, 0.7, 0.57), cell_k = floor((x_k - lo_k) / h).  A = the points selected so far, U = the unselected
points with dist2 >= r2 to every point of A.  Until U is empty: in every non-empty cell the point of U with the
smallest key is the winner; the winners are visited in ascending key order and one is accepted iff its dist2 to
every winner accepted in this round is >= r2; the accepted join A, and every point of U with dist2 < r2 to an
accepted one leaves U.  A level's points are appended sorted by key; what is left after level 19 (or when r2 is
no longer a normal number) is the tail, level 20, sorted by key.
"""
import itertools

import numpy as np

LEVELS = 19
TAIL = 20
CELL_FACTOR = {1: 0.5, 2: 0.7, 3: 0.57}
DBL_MIN = 2.2250738585072014e-308


def mix32(h):
    h = np.asarray(h, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def keys(n, seed=0):
    i = np.arange(n, dtype=np.uint64)
    off = np.uint64((int(seed) * 0x9E3779B9) & 0xFFFFFFFF)
    return (mix32((i + off) & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | i


def dist2(a, b):
    """Squared distances of the rows of a to the rows of b (broadcast), summed in axis order."""
    d = a[..., 0] - b[..., 0]
    s = d * d
    for k in range(1, a.shape[-1]):
        d = a[..., k] - b[..., k]
        s = s + d * d
    return s


def _pack(cells):
    p = cells[:, 0].astype(np.int64)
    for k in range(1, cells.shape[1]):
        p = p | (cells[:, k].astype(np.int64) << np.int64(21 * k))
    return p


class _CellMap:
    """Points stored by cell, at most one per cell; `near(x, cells)` is the smallest dist2 of every query to the
    stored points in the 5^d cells around its own (inf where there is none)."""

    def __init__(self, coords, idx, cells):
        packed = _pack(cells)
        order = np.argsort(packed, kind="stable")
        self.packed, self.idx, self.coords = packed[order], np.asarray(idx)[order], coords
        assert np.all(np.diff(self.packed) > 0), "two stored points share a cell"

    def near(self, x, cells):
        best = np.full(len(x), np.inf)
        if len(self.packed) == 0 or len(x) == 0:
            return best
        d = cells.shape[1]
        for off in itertools.product(range(-2, 3), repeat=d):
            nc = cells + np.asarray(off, dtype=np.int64)
            ok = np.all(nc >= 0, axis=1)
            p = _pack(np.where(ok[:, None], nc, 0))
            at = np.minimum(np.searchsorted(self.packed, p), len(self.packed) - 1)
            hit = ok & (self.packed[at] == p)
            if hit.any():
                d2 = dist2(x[hit], self.coords[self.idx[at[hit]]])
                best[hit] = np.minimum(best[hit], d2)
        return best


def order_maxmin(coords, seed=0, stats=None):
    """(perm int64 (n,), level int32 (n,) by position) of the definition above."""
    x = np.ascontiguousarray(coords, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] not in (1, 2, 3) or x.shape[0] < 1:
        raise ValueError("coords must be (n >= 1, d) with d in 1, 2, 3")
    if not np.all(np.isfinite(x)):
        raise ValueError("coords must be finite")
    n, d = x.shape
    key = keys(n, seed)
    lo, hi = x.min(axis=0), x.max(axis=0)
    c = 0.5 * (lo + hi)
    p1 = int(np.argmin(dist2(x, c[None, :])))  # argmin returns the first (smallest) index of the minimum
    R2 = dist2(x, x[p1][None, :]).max()
    if not np.isfinite(R2):
        raise ValueError("squared distances overflow")
    R = np.sqrt(R2)
    level = np.full(n, TAIL, dtype=np.int32)
    level[p1] = 0
    for l in range(1, LEVELS + 1):
        if np.all(level != TAIL):
            break
        r = np.ldexp(R, -l)
        r2 = r * r
        h = r * CELL_FACTOR[d]
        if not (r2 >= DBL_MIN):
            break
        cells = np.floor((x - lo[None, :]) / h).astype(np.int64)
        sel = np.flatnonzero(level != TAIL)
        A = _CellMap(x, sel, cells[sel])
        uns = np.flatnonzero(level == TAIL)
        U = uns[A.near(x[uns], cells[uns]) >= r2]
        rounds = 0
        while U.size:
            rounds += 1
            # the winner of every non-empty cell: U in key order, the first of each cell
            by_key = U[np.argsort(key[U], kind="stable")]
            pc = _pack(cells[by_key])
            _, first = np.unique(pc, return_index=True)
            winners = by_key[np.sort(first)]  # ascending key
            # cells shifted by 2 and packed, so that a neighbour cell is one integer addition away
            offs = [int(sum(o << (21 * k) for k, o in enumerate(off))) for off in itertools.product(range(-2, 3), repeat=d)]
            wcell = [int(v) for v in _pack(cells[winners] + 2)]
            accepted = {}  # packed cell -> point
            for w, cw in zip(winners.tolist(), wcell):
                ok = True
                for o in offs:
                    v = accepted.get(cw + o)
                    if v is not None and dist2(x[w], x[v]) < r2:
                        ok = False
                        break
                if ok:
                    accepted[cw] = w
            acc = np.fromiter(accepted.values(), dtype=np.int64, count=len(accepted))
            level[acc] = l
            keep = _CellMap(x, acc, cells[acc]).near(x[U], cells[U]) >= r2
            U = U[keep]
        if stats is not None:
            stats.setdefault("rounds", {})[l] = rounds
    perm = np.lexsort((key, level)).astype(np.int64)
    return perm, level[perm]


def order_random(n, seed=0):
    return np.argsort(keys(n, seed), kind="stable").astype(np.int64)


def greedy_maxmin(coords, start):
    """The exact greedy max-min order from `start` (O(n^2)): every next point is the one farthest from the points
    before it (ties to the smallest index).  Returns (perm, g) with g[k] the distance of point k to its
    predecessors (g[0] = inf)."""
    x = np.ascontiguousarray(coords, dtype=np.float64)
    n = x.shape[0]
    perm = np.empty(n, dtype=np.int64)
    g = np.empty(n)
    perm[0], g[0] = start, np.inf
    near = dist2(x, x[start][None, :])
    near[start] = -1.0
    for k in range(1, n):
        j = int(np.argmax(near))
        perm[k], g[k] = j, np.sqrt(near[j])
        near = np.minimum(near, dist2(x, x[j][None, :]))
        near[perm[: k + 1]] = -1.0
    return perm, g


def predecessor_dist2(coords, perm, block=512):
    """s2[k] = min dist2 of point perm[k] to perm[:k] (inf for k = 0), by blocked brute force."""
    x = np.ascontiguousarray(coords, dtype=np.float64)[perm]
    n = x.shape[0]
    s2 = np.full(n, np.inf)
    for a in range(0, n, block):
        b = min(n, a + block)
        d2 = dist2(x[a:b, None, :], x[None, :b, :])  # (rows a..b) x (points 0..b)
        mask = np.arange(b)[None, :] < np.arange(a, b)[:, None]
        s2[a:b] = np.where(mask, d2, np.inf).min(axis=1)
    return s2


def level_radii(coords, perm):
    """(R, r2 per level 0 .. 19 (index 0: inf)) of the order's own arithmetic."""
    x = np.ascontiguousarray(coords, dtype=np.float64)
    R = np.sqrt(dist2(x, x[perm[0]][None, :]).max())
    r2 = np.full(LEVELS + 1, np.inf)
    for l in range(1, LEVELS + 1):
        r = np.ldexp(R, -l)
        r2[l] = r * r
    return R, r2


def check_properties(coords, perm, level):
    """Assert the order's defining properties, in the restatement's own arithmetic: perm is a permutation whose
    levels do not decrease; every point of a level l <= 19 has dist2 >= r_l^2 to all of its predecessors
    (separation); after level l every later point has a point of levels <= l at dist2 < r_l^2 (covering).  A
    k-d tree proposes the pairs and the nearest points; dist2 above decides."""
    from scipy.spatial import cKDTree

    x = np.ascontiguousarray(coords, dtype=np.float64)
    n = x.shape[0]
    perm, level = np.asarray(perm), np.asarray(level)
    assert perm.shape == (n,) and level.shape == (n,)
    assert np.array_equal(np.sort(perm), np.arange(n)), "not a permutation"
    assert level[0] == 0 and np.all(np.diff(level) >= 0) and (n == 1 or level[1] >= 1)
    assert level.min() >= 0 and level.max() <= TAIL
    R, r2 = level_radii(x, perm)
    xp = x[perm]
    for l in range(1, LEVELS + 1):
        n_l = int(np.searchsorted(level, l, side="right"))  # the points of levels <= l
        if not r2[l] >= DBL_MIN:
            assert n_l == int(np.searchsorted(level, l - 1, side="right")), "a level past the last radius"
            continue
        tree = cKDTree(xp[:n_l])
        pairs = tree.query_pairs(np.ldexp(R, -l) * (1.0 + 1e-9), output_type="ndarray")
        if len(pairs):
            late = level[pairs.max(axis=1)] == l
            pr = pairs[late]
            assert np.all(dist2(xp[pr[:, 0]], xp[pr[:, 1]]) >= r2[l]), f"separation fails at level {l}"
        if n_l < n:
            _, at = tree.query(xp[n_l:])
            assert np.all(dist2(xp[n_l:], xp[at]) < r2[l]), f"covering fails at level {l}"


# ---------------------------------------------------------------- the inputs the host and GPU tests share
def inputs():
    """name -> coords: uniform points in 1, 2 and 3 dimensions, a 32 x 32 integer lattice (exact ties at r), 300
    points with 100 of them repeated, and the degenerate sets."""
    out = {}
    for d in (1, 2, 3):
        out[f"uniform{d}d"] = np.random.default_rng(100 + d).uniform(size=(1500, d))
    g = np.arange(32, dtype=np.float64)
    out["lattice32"] = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    rng = np.random.default_rng(7)
    base = rng.uniform(size=(300, 2))
    out["duplicates"] = np.concatenate([base, base[rng.choice(300, size=100, replace=False)]])
    out["one"] = np.array([[0.25, 0.5]])
    out["two"] = np.array([[0.0, 0.0], [1.0, 0.5]])
    out["coincident"] = np.tile(np.array([[0.3, 0.7, 0.1]]), (50, 1))
    return out


_INPUTS = None
_REFERENCE = {}


def case(name):
    global _INPUTS
    if _INPUTS is None:
        _INPUTS = inputs()
    return _INPUTS[name]


def reference(name, seed=0):
    """(perm, level) of the restatement for a shared input, computed once per process and not to be modified."""
    if (name, seed) not in _REFERENCE:
        perm, level = order_maxmin(case(name), seed)
        perm.setflags(write=False)
        level.setflags(write=False)
        _REFERENCE[(name, seed)] = (perm, level)
    return _REFERENCE[(name, seed)]


def greedy_ratio(coords, perm, level):
    """min and median over the non-tail positions k >= 1 of s_k / g_k: the distance of point k to its predecessors
    over the same for the exact greedy max-min order started at perm[0]."""
    s2 = predecessor_dist2(coords, perm)
    _, g = greedy_maxmin(coords, int(perm[0]))
    body = np.asarray(level) <= LEVELS
    body[0] = False
    ratio = np.sqrt(s2[body]) / g[body]
    return float(ratio.min()), float(np.median(ratio))
