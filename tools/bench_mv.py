#!/usr/bin/env python3
"""Time the multivariate (coregionalised) sweep nngp_bf_sweep_mv in one process.

N = 1e6 points in 2-D, exponential, (q, m) = (2, 15), (2, 31), (3, 20), (4, 15): the sweep likelihood-only and with B
written, against
  1. the only other route to this model: the dense joint blocks built in torch, torch.linalg.cholesky on the
     (rows, n, n) batch in chunks that fit memory, and a triangular solve.  It is timed on --torch-rows rows (all of
     them by default) starting at row 64, and the figure per 1e6 rows is that time scaled by rows;
  2. nngp_bf_sweep_noise at the same m on one outcome with unit weights: the price per row of one response.
The log-likelihood terms of the two routes are compared on the rows the torch route ran.
Warm clocks, untimed launches of each first, event-bracketed rounds that alternate the candidates; medians, minima
and maxima.  Prints one JSON line and writes it to profiles/mv/bench_mv.json."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pynngp_amd import _lib  # noqa: E402

AFULL = np.array([[1.0, 0, 0, 0], [0.5, 0.9, 0, 0], [0.3, 0.6, 0.8, 0], [0.7, 0.4, 0.35, 0.95]])


def time_ms(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def torch_route(coords, nbr, Y, A, phi, tau2, lo, hi, chunk):
    """(sum 2 log diag LF, sum |E|^2) over rows [lo, hi) from dense joint Cholesky factors: the last q rows of the
    joint factor are [W, LF], and of the whitened joint values LF^-1 (y - W z_N)."""
    q = A.shape[0]
    outer = torch.stack([torch.outer(A[:, k], A[:, k]) for k in range(q)])  # (q, q, q)
    ld = torch.zeros((), dtype=torch.float64, device=coords.device)
    qd = torch.zeros_like(ld)
    for a in range(lo, hi, chunk):
        b = min(a + chunk, hi)
        idx = nbr[a:b].long()
        pts = torch.cat([coords[idx], coords[a:b, None]], 1)
        # (torch.cdist switches to |a|^2 + |b|^2 - 2 a.b above 25 rows, which cancels for close points)
        t = pts[:, :, None, :] - pts[:, None, :, :]
        d = torch.sqrt((t * t).sum(-1))
        n = pts.shape[1] * q
        C = sum(torch.exp(-phi[k] * d)[:, :, None, :, None] * outer[k][None, None, :, None, :] for k in range(q))
        C = C.reshape(b - a, n, n) + torch.diag(tau2.repeat(pts.shape[1]))
        L = torch.linalg.cholesky(C)
        y = torch.cat([Y[idx], Y[a:b, None]], 1).reshape(b - a, n, 1)
        z = torch.linalg.solve_triangular(L, y, upper=False)
        ld += 2.0 * torch.log(torch.diagonal(L, dim1=1, dim2=2)[:, -q:]).sum()
        qd += (z[:, -q:, 0] ** 2).sum()
    return ld, qd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--shapes", default="2,15 2,31 3,20 4,15")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-rows", type=int, default=0, help="rows of the torch route (0: all)")
    ap.add_argument("--torch-chunk", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv", "bench_mv.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mv needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    lib = _lib.load()
    kind = "exponential"
    coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, 2))).to(dev)
    one = torch.ones(a.n, dtype=torch.float64, device=dev)
    lo = 64
    hi = a.n if a.torch_rows <= 0 else min(a.n, lo + a.torch_rows)
    out = []
    for q, m in [tuple(int(x) for x in s.split(",")) for s in a.shapes.split()]:
        A = AFULL[:q, :q]
        phi = 30.0 + 25.0 * np.arange(q)
        tau2 = 0.05 * (1 + np.arange(q))
        Y = torch.from_numpy(rng.standard_normal((a.n, q, 1))).to(dev)
        nbr = _lib.knn_prior(coords, m)
        ws = _lib._workspace(lib.nngp_bf_sweep_mv_workspace_bytes(a.n, m, q), dev)
        wsn = _lib._workspace(lib.nngp_bf_sweep_noise_workspace_bytes(a.n, m), dev)
        y1 = Y[:, 0, 0].contiguous()
        At, pt, tt = (torch.tensor(x, dtype=torch.float64, device=dev) for x in (A, phi, tau2))

        def lik():
            return _lib.bf_sweep_mv(coords, nbr, 0, kind, A, phi, tau2, Y, want_b=False, want_lf=False, workspace=ws)

        def with_b():
            return _lib.bf_sweep_mv(coords, nbr, 0, kind, A, phi, tau2, Y, want_b=True, want_lf=True, workspace=ws)

        def noise():
            return _lib.bf_sweep_noise(coords, nbr, 0, kind, 1.0, float(phi[0]), float(tau2[0]), one, values=y1,
                                       want_bf=False, workspace=wsn)

        def dense():
            return torch_route(coords, nbr, Y[:, :, 0], At, pt, tt, lo, hi, a.torch_chunk)

        cands = {"mv": lik, "mv_b": with_b, "noise_1": noise}
        for fn in cands.values():
            time_ms(fn, a.warmup)
        time_ms(dense, 1)
        t = {k: [] for k in list(cands) + ["torch"]}
        for _ in range(a.rounds):
            for k, fn in cands.items():
                t[k].append(time_ms(fn, a.launches))
            t["torch"].append(time_ms(dense, 1) * a.n / (hi - lo))
        med = {k: float(np.median(x)) for k, x in t.items()}
        sub = _lib.bf_sweep_mv(coords, nbr[lo:hi].contiguous(), lo, kind, A, phi, tau2, Y, want_b=False,
                               want_lf=False)[3].cpu().numpy()
        ld, qd = (float(x) for x in dense())
        row = {"q": q, "m": m, "n_joint": (m + 1) * q, "torch_rows": hi - lo,
               **{k + "_ms": x for k, x in med.items()}, **{k + "_ms_min": min(x) for k, x in t.items()},
               **{k + "_ms_max": max(x) for k, x in t.items()},
               "torch_over_mv": med["torch"] / med["mv"], "torch_over_mv_b": med["torch"] / med["mv_b"],
               "mv_over_noise_1": med["mv"] / med["noise_1"],
               "loglik_terms_rel_diff_mv_vs_torch": abs((sub[0] + sub[1]) - (ld + qd)) / abs(ld + qd),
               "flags": [float(sub[2]), float(sub[3])]}
        out.append(row)
        print(json.dumps(row), flush=True)
    res = {"tool": "bench_mv", "n": a.n, "kind": kind, "launches": a.launches, "rounds": a.rounds, "warmup": a.warmup,
           "torch_chunk": a.torch_chunk, "device": torch.cuda.get_device_name(0), "results": out}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
