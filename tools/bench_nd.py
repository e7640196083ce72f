#!/usr/bin/env python3
"""Time the 4 .. 16-dimensional path (nngp_knn_prior_nd, nngp_bf_sweep_nd, nngp_bf_grad_nd) in one process.

Neighbour build: nngp_knn_prior_nd at d = 8, m = 15 for every row at N = 1e5 and, at N = 1e6, for two sampled row
ranges (the middle and the last rows, the heaviest), beside sklearn's KDTree (NearestNeighbors, kd_tree, n_jobs = 16)
answering the same number of unrestricted queries on the same points.

Sweeps at N = 1e6, d = 4, 8, 16, m = 15, 20, against
  1. the only earlier route to such data: a CallableCovariance with a broadcasting torch callable, its joint blocks
     materialised and factorised by nngp_bf_sweep_blocks (recorded as unavailable with the error if it refuses);
  2. nngp_bf_sweep_noise / nngp_bf_grad_noise at dim 3 (the first three columns, unit weights) on the same
     neighbour indices: the price of the extra axes.
The sweeps' neighbour sets are exact prior sets inside consecutive chunks of --chunk points (an exact build of 1e6
rows is the first measurement's subject, not this one's); the same indices serve every candidate.
Warm clocks, untimed launches of each first, event-bracketed rounds that alternate the candidates; medians.
Prints one JSON line and writes it to profiles/nd/bench_nd.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pynngp_amd import _lib  # noqa: E402
from pynngp_amd.nngp import CallableCovariance  # noqa: E402


def time_ms(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def chunked_sets(coords, m, chunk):
    """Exact prior neighbour sets inside consecutive chunks of ``chunk`` points."""
    out = []
    for lo in range(0, coords.shape[0], chunk):
        nb = _lib.knn_prior_nd(coords[lo:lo + chunk].contiguous(), m)
        out.append(torch.where(nb >= 0, nb + lo, nb))
    return torch.cat(out).contiguous()


def knn_part(a, dev, rng):
    res = []
    d, m = 8, 15
    for n, ranges in ((100_000, [(0, 100_000)]), (1_000_000, [(500_000, 500_000 + a.knn_rows),
                                                             (1_000_000 - a.knn_rows, 1_000_000)])):
        host = rng.uniform(0.0, 1.0, (n, d))
        c = torch.from_numpy(host).to(dev)
        _lib.knn_prior_nd(c, m, 0, 4096)  # warm-up
        torch.cuda.synchronize()
        from sklearn.neighbors import NearestNeighbors

        t0 = time.perf_counter()
        tree = NearestNeighbors(n_neighbors=m, algorithm="kd_tree", n_jobs=16).fit(host)
        t_build = time.perf_counter() - t0
        for q0, q1 in ranges:
            ts = []
            for _ in range(a.knn_rounds):
                ts.append(time_ms(lambda: _lib.knn_prior_nd(c, m, q0, q1), 1))
            nq = min(q1 - q0, a.kdtree_rows)
            t0 = time.perf_counter()
            tree.kneighbors(host[q1 - nq:q1])
            t_q = time.perf_counter() - t0
            res.append({"n": n, "dim": d, "m": m, "rows": [q0, q1], "sampled": (q1 - q0) < n,
                        "knn_prior_nd_ms": float(np.median(ts)), "knn_prior_nd_us_per_row": float(np.median(ts)) * 1e3 / (q1 - q0),
                        "kdtree_build_s": t_build, "kdtree_query_rows": nq, "kdtree_query_us_per_row": t_q * 1e6 / nq})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--m", type=int, nargs="+", default=[15, 20])
    ap.add_argument("--kind", default="exponential")
    ap.add_argument("--chunk", type=int, default=20_000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--blocks-warmup", type=int, default=3)
    ap.add_argument("--blocks-launches", type=int, default=2)
    ap.add_argument("--knn-rows", type=int, default=8192)
    ap.add_argument("--knn-rounds", type=int, default=3)
    ap.add_argument("--kdtree-rows", type=int, default=8192)
    ap.add_argument("--skip-knn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nd", "bench_nd.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nd needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    lib = _lib.load()
    knn = [] if a.skip_knn else knn_part(a, dev, rng)
    y = torch.from_numpy(rng.standard_normal(a.n)).to(dev)
    one = torch.ones(a.n, dtype=torch.float64, device=dev)
    s2, t2 = 1.0, 0.1
    out = []
    for d in a.dims:
        coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, d))).to(dev)
        c3 = coords[:, :3].contiguous()
        phi = [float(x) for x in (0.6 + 0.1 * np.arange(d)) / np.sqrt(d / 4.0)]
        pt = torch.tensor(phi, dtype=torch.float64, device=dev)

        def ard_matrix(x, z):  # sigma2 exp(-|phi (x - z)|) on (.., ka, d) x (.., kb, d) rows: (.., ka, kb)
            dd = (x[..., :, None, :] - z[..., None, :, :]) * pt
            return s2 * torch.exp(-torch.sqrt((dd * dd).sum(-1)))

        for m in a.m:
            nbr = chunked_sets(coords, m, a.chunk)
            ws = _lib._workspace(lib.nngp_bf_sweep_nd_workspace_bytes(a.n, m, d), dev)
            wsn = _lib._workspace(lib.nngp_bf_sweep_noise_workspace_bytes(a.n, m), dev)
            wsg = _lib._workspace(lib.nngp_bf_grad_workspace_bytes(a.n, m), dev)

            def nd():
                return _lib.bf_sweep_nd(coords, nbr, 0, a.kind, s2, phi, t2, values=y, want_bf=False, workspace=ws)

            def gnd():
                return _lib.bf_grad_nd(coords, nbr, 0, a.kind, s2, phi, t2, y, workspace=ws)

            def noise():
                return _lib.bf_sweep_noise(c3, nbr, 0, a.kind, s2, phi[0], t2, one, values=y, want_bf=False,
                                           workspace=wsn)

            def gnoise():
                return _lib.bf_grad_noise(c3, nbr, 0, a.kind, s2, phi[0], t2, y, one, workspace=wsg)

            blocks, blocks_error = None, None
            try:
                cv = CallableCovariance(ard_matrix, tau2=t2)
                wsb = _lib._workspace(lib.nngp_bf_sweep_blocks_workspace_bytes(a.n), dev)
                pb = torch.empty(4, dtype=torch.float64, device=dev)

                def blocks():
                    blk = cv.blocks(coords, nbr, 0)
                    return _lib.bf_sweep_blocks(blk, nbr, a.n, 0, values=y, qvalues=y, want_bf=False, workspace=wsb,
                                                partials=pb)

                blocks()
                torch.cuda.synchronize()
            except Exception as e:  # the route refuses these columns: recorded, not hidden
                blocks, blocks_error = None, f"{type(e).__name__}: {e}"[:300]
            cands = {"nd": nd, "noise_d3": noise, "grad_nd": gnd, "grad_noise_d3": gnoise}
            for fn in cands.values():
                time_ms(fn, a.warmup)
            if blocks is not None:
                time_ms(blocks, a.blocks_warmup)
            t = {k: [] for k in list(cands) + (["callable"] if blocks is not None else [])}
            for _ in range(a.rounds):
                for k, fn in cands.items():
                    t[k].append(time_ms(fn, a.launches))
                if blocks is not None:
                    t["callable"].append(time_ms(blocks, a.blocks_launches))
            med = {k: float(np.median(x)) for k, x in t.items()}
            row = {"dim": d, "m": m, **{k + "_ms": x for k, x in med.items()},
                   **{k + "_ms_min": min(x) for k, x in t.items()},
                   "nd_over_noise_d3": med["nd"] / med["noise_d3"],
                   "grad_nd_over_grad_noise_d3": med["grad_nd"] / med["grad_noise_d3"],
                   "grad_nd_over_nd": med["grad_nd"] / med["nd"], "central_difference_sweeps": 2 * (d + 2)}
            if blocks is not None:
                pn = nd()[3].cpu().numpy()
                blocks()
                pbh = pb.cpu().numpy()
                row["callable_over_nd"] = med["callable"] / med["nd"]
                row["loglik_rel_diff_nd_vs_callable"] = float(abs((pn[0] + pn[1]) - (pbh[0] + pbh[1])) /
                                                              abs(pbh[0] + pbh[1]))
            else:
                row["callable_error"] = blocks_error
            out.append(row)
            print(json.dumps(row), flush=True)
    res = {"tool": "bench_nd", "n": a.n, "kind": a.kind, "chunk": a.chunk, "launches": a.launches, "rounds": a.rounds,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "knn": knn, "results": out}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
