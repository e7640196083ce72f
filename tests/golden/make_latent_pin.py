"""Generate tests/golden/latent_single_pin.npz: what the single-RHS latent calls compute, inputs and outputs both.

Run by hand on a GPU, from the repository root, on the commit whose bits are to be pinned (the fixture in the
tree was written by commit dd168c1, the last one with separate single-RHS kernels)::

    python tests/golden/make_latent_pin.py

It calls only ``_lib.reverse_neighbors``, ``_lib.gibbs_prepare``, ``_lib.precision_apply``,
``_lib.precision_sqrt_t_apply`` and ``_lib.latent_cg``.  tests/test_gpu_latent_pin.py replays the stored inputs
and asserts equality of every stored output, so it needs nothing from this file.

Layout (flat npz keys; G a geometry name, T in {"d0", "d1"} = without / with the diagonal term):
  sigma2                    scalar
  geom_names, cg_names      arrays of names
  G.nbr, G.B, G.F           the DAG and its unit-variance factors
  op.G.x, .z2, .d           operator inputs (z1 = x; T = d0 uses x alone)
  op.G.T.apply, .sqrt       precision_apply(x) and precision_sqrt_t_apply(x, z2)
  rhs.G.d, rhs.G.b          the diagonal term and the right-hand side of the solves on geometry G
  cg.C.geom, .rtol, .max_iter, .check_every    solver inputs of case C (check_every: every value that was run,
                            all with the one stored result); .x0 if the start is not zero; .b if not rhs.G.b
  cg.C.x, .info             the solution as returned and the four info words
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import nngp_oracle as O  # noqa: E402
from pynngp_amd import _lib  # noqa: E402

SIGMA2 = 1.3
LONG_LIST = 512  # latent.hip's kLongList: a longer reverse list is summed by the whole block


def field(n, m):
    """Uniform 2-D coordinates, oracle neighbour sets and oracle unit-variance exponential B / F."""
    c = np.random.default_rng(0).uniform(size=(n, 2))
    nbr = O.knn_prior(c, m)
    B, F, _ = O.bf_sweep(c, nbr, "exponential", (1.0, 6.0, 0.0))
    return nbr, B, F


def handmade(nbr, rng):
    n, m = nbr.shape
    return nbr, rng.uniform(-0.3, 0.3, (n, m)), rng.uniform(0.1, 2.0, n)


def holes():
    """Rows whose valid slots are not a prefix (-1 in the middle), random B in the -1 slots too."""
    rng = np.random.default_rng(3)
    n, m = 300, 6
    nbr = np.full((n, m), -1, dtype=np.int32)
    for j in range(1, n):
        slots = rng.choice(m, size=int(rng.integers(1, min(m, j) + 1)), replace=False)
        nbr[j, slots] = rng.choice(j, size=len(slots), replace=False)
    assert np.any((nbr[:, :-1] < 0) & (nbr[:, 1:] >= 0))
    return handmade(nbr, rng)


def two_hubs():
    """Every row j >= 2 has parents 0 and 1: two reverse lists of 598 entries in the first column-phase tile,
    so the block-cooperative sum runs twice in one tile."""
    rng = np.random.default_rng(4)
    n, m = 600, 4
    nbr = np.full((n, m), -1, dtype=np.int32)
    for j in range(2, n):
        nbr[j, :2] = (0, 1)
        k = min(m - 2, j - 2)
        if k > 0:
            nbr[j, 2:2 + k] = 2 + rng.choice(j - 2, size=k, replace=False)
    deg = np.bincount(nbr[nbr >= 0], minlength=n)
    assert deg[0] == deg[1] == n - 2 > LONG_LIST and deg[2:].max() <= LONG_LIST
    return handmade(nbr, rng)


def random_d(rng, n):
    return rng.uniform(0.1, 10.0, n) * (rng.uniform(size=n) >= 0.3)  # 30 % zeros


def main():
    dev = torch.device("cuda", 0)
    dt = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    geoms = {"f1_1": field(1, 1), "f257_32": field(257, 32), "f400_4": field(400, 4), "f400_8": field(400, 8),
             "holes300_6": holes(), "twohub600_4": two_hubs()}
    out = {"sigma2": np.float64(SIGMA2), "geom_names": np.array(list(geoms))}
    device_geom = {}
    for g, (nbr, B, F) in geoms.items():
        nbr = np.ascontiguousarray(nbr, dtype=np.int32)
        out[f"{g}.nbr"], out[f"{g}.B"], out[f"{g}.F"] = nbr, np.array(B, dtype=np.float64), np.array(F, dtype=np.float64)
        nbr_d, B_d = dt(nbr), dt(out[f"{g}.B"])
        off, rev_j, rev_k = _lib.reverse_neighbors(nbr_d)
        prep = _lib.gibbs_prepare(B_d, dt(out[f"{g}.F"]), off, rev_j, rev_k)
        device_geom[g] = (nbr_d, B_d, off, rev_j, rev_k, prep, SIGMA2)

    rng = np.random.default_rng(2024)
    for g, geom in device_geom.items():
        n = geoms[g][0].shape[0]
        x, z2, d = rng.standard_normal(n), rng.standard_normal(n), random_d(rng, n)
        if n > 1:
            assert np.any(d == 0) and np.any(d > 0)
        out[f"op.{g}.x"], out[f"op.{g}.z2"], out[f"op.{g}.d"] = x, z2, d
        out[f"op.{g}.d0.apply"] = _lib.precision_apply(*geom, dt(x)).cpu().numpy()
        out[f"op.{g}.d0.sqrt"] = _lib.precision_sqrt_t_apply(*geom, dt(x)).cpu().numpy()
        out[f"op.{g}.d1.apply"] = _lib.precision_apply(*geom, dt(x), d=dt(d)).cpu().numpy()
        out[f"op.{g}.d1.sqrt"] = _lib.precision_sqrt_t_apply(*geom, dt(x), dt(z2), d=dt(d)).cpu().numpy()

    for g in ("f400_8", "twohub600_4"):
        n = geoms[g][0].shape[0]
        out[f"rhs.{g}.d"], out[f"rhs.{g}.b"] = random_d(rng, n), rng.standard_normal(n)
    b_nan = out["rhs.f400_8.b"].copy()
    b_nan[17] = np.nan
    cg = {"f400_8": dict(geom="f400_8", rtol=1e-8, max_iter=1000, check_every=[1, 8]),
          "twohub600_4": dict(geom="twohub600_4", rtol=1e-8, max_iter=1000, check_every=[1, 8]),
          "x0": dict(geom="f400_8", rtol=1e-8, max_iter=1000, check_every=[8], x0=rng.standard_normal(400)),
          "max_iter3": dict(geom="f400_8", rtol=1e-10, max_iter=3, check_every=[8]),
          "nan_b": dict(geom="f400_8", rtol=1e-8, max_iter=1000, check_every=[8], b=b_nan)}
    out["cg_names"] = np.array(list(cg))
    for name, k in cg.items():
        g = k["geom"]
        b, x0 = k.get("b", out[f"rhs.{g}.b"]), k.get("x0", np.zeros_like(out[f"rhs.{g}.b"]))
        runs = [_lib.latent_cg(*device_geom[g], dt(b), dt(x0), d=dt(out[f"rhs.{g}.d"]), rtol=k["rtol"],
                               max_iter=k["max_iter"], check_every=ce) for ce in k["check_every"]]
        x, info = runs[0][0].cpu().numpy(), np.array(runs[0][1])
        for xr, ir in runs[1:]:  # the chunking of the host's reads changes nothing
            assert np.array_equal(xr.cpu().numpy(), x) and np.array_equal(np.array(ir), info, equal_nan=True)
        print(f"cg {name}: info {info.tolist()}")
        for key, v in k.items():
            out[f"cg.{name}.{key}"] = np.array(v)
        out[f"cg.{name}.x"], out[f"cg.{name}.info"] = x, info
    info = {name: out[f"cg.{name}.info"] for name in cg}
    assert info["f400_8"][1] == info["twohub600_4"][1] == info["x0"][1] == 1.0
    assert info["max_iter3"].tolist()[:2] == [3.0, 0.0] and info["nan_b"][1] == -1.0

    path = os.path.join(HERE, "latent_single_pin.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
