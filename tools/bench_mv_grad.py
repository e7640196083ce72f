#!/usr/bin/env python3
"""Time the multivariate gradient sweep nngp_bf_grad_mv beside the sweeps it replaces, in one process.

N = 1e6 points in 2-D, exponential, (q, m) = (2, 15), (2, 31), (3, 20), (4, 15) (tools/bench_mv.py's model and
protocol): the gradient sweep, the likelihood-only sweep and the sweep with B written, of the same build.  A
central-difference gradient costs 2 P likelihood-only sweeps, P = q (q + 1) / 2 + 2 q; that figure is the measured
likelihood-only time scaled by 2 P.  Warm clocks, untimed launches of each first, event-bracketed rounds that alternate
the candidates; medians, minima and maxima.  Prints one JSON line and writes it to profiles/mv/bench_mv_grad.json."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pynngp_amd import _lib  # noqa: E402
from tools.bench_mv import AFULL, time_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--shapes", default="2,15 2,31 3,20 4,15")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv", "bench_mv_grad.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mv_grad needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    lib = _lib.load()
    kind = "exponential"
    coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, 2))).to(dev)
    out = []
    for q, m in [tuple(int(x) for x in s.split(",")) for s in a.shapes.split()]:
        A, phi, tau2 = AFULL[:q, :q], 30.0 + 25.0 * np.arange(q), 0.05 * (1 + np.arange(q))
        npar = q * (q + 1) // 2 + 2 * q
        Y = torch.from_numpy(rng.standard_normal((a.n, q, 1))).to(dev)
        nbr = _lib.knn_prior(coords, m)
        ws = _lib._workspace(lib.nngp_bf_grad_mv_workspace_bytes(a.n, m, q), dev)

        def grad():
            return _lib.bf_grad_mv(coords, nbr, 0, kind, A, phi, tau2, Y, workspace=ws)

        def lik():
            return _lib.bf_sweep_mv(coords, nbr, 0, kind, A, phi, tau2, Y, want_b=False, want_lf=False, workspace=ws)

        def with_b():
            return _lib.bf_sweep_mv(coords, nbr, 0, kind, A, phi, tau2, Y, want_b=True, want_lf=True, workspace=ws)

        cands = {"grad": grad, "mv": lik, "mv_b": with_b}
        for fn in cands.values():
            time_ms(fn, a.warmup)
        t = {k: [] for k in cands}
        for _ in range(a.rounds):
            for k, fn in cands.items():
                t[k].append(time_ms(fn, a.launches))
        med = {k: float(np.median(x)) for k, x in t.items()}
        pg, pl = grad()[0].cpu().numpy(), lik()[3].cpu().numpy()
        row = {"q": q, "m": m, "n_joint": (m + 1) * q, "n_params": npar,
               **{k + "_ms": x for k, x in med.items()}, **{k + "_ms_min": min(x) for k, x in t.items()},
               **{k + "_ms_max": max(x) for k, x in t.items()},
               "grad_over_mv_b": med["grad"] / med["mv_b"], "grad_over_mv": med["grad"] / med["mv"],
               "central_differences_ms": 2 * npar * med["mv"],
               "central_differences_over_grad": 2 * npar * med["mv"] / med["grad"],
               "loglik_terms_rel_diff_grad_vs_mv": abs((pg[0] + pg[1]) - (pl[0] + pl[1])) / abs(pl[0] + pl[1]),
               "flags": [float(pg[2]), float(pg[3])]}
        out.append(row)
        print(json.dumps(row), flush=True)
    res = {"tool": "bench_mv_grad", "n": a.n, "kind": kind, "launches": a.launches, "rounds": a.rounds,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "results": out}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
