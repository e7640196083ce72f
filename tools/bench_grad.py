#!/usr/bin/env python3
"""Time the gradient sweep (nngp_bf_grad) against the forward log-likelihood sweep (bf_sweep, B / F off) in one
process: warm clocks, >= 200 untimed launches of each first, event-bracketed rounds that alternate the two.
Prints one JSON line.  python tools/bench_grad.py [--n 1000000] [--m 15 20] [--kind exponential]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pynngp_amd import _lib  # noqa: E402


def time_ms(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, nargs="+", default=[15, 20])
    ap.add_argument("--kind", default="exponential")
    ap.add_argument("--theta", type=float, nargs=3, default=[1.0, 30.0, 0.1])
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, 2))).to(dev)
    y = torch.from_numpy(rng.standard_normal(a.n)).to(dev)
    out = []
    for m in a.m:
        nbr = _lib.knn_prior(coords, m)
        order, nbs = _lib.row_order(coords, 0, a.n, nbr)
        wsf = _lib._workspace(_lib.load().nngp_bf_sweep_workspace_bytes(a.n, m, _lib.KIND_CODES[a.kind], 2, 0), dev)
        wsg = _lib._workspace(_lib.load().nngp_bf_grad_workspace_bytes(a.n, m), dev)
        pf = torch.empty(4, dtype=torch.float64, device=dev)

        def fwd():
            return _lib.bf_sweep(coords, nbs, 0, a.kind, *a.theta, values=y, want_bf=False, partials=pf,
                                 workspace=wsf, order=order)

        def grad():
            return _lib.bf_grad(coords, nbs, 0, a.kind, *a.theta, y, order=order, workspace=wsg)

        time_ms(fwd, a.warmup)
        time_ms(grad, a.warmup)
        tf, tg = [], []
        for _ in range(a.rounds):
            tf.append(time_ms(fwd, a.launches))
            tg.append(time_ms(grad, a.launches))
        p, g, _ = grad()
        pfh, ph = pf.cpu().numpy(), p.cpu().numpy()
        f, gr = float(np.median(tf)), float(np.median(tg))
        out.append({"m": m, "forward_ms": f, "forward_ms_min": min(tf), "grad_ms": gr, "grad_ms_min": min(tg),
                    "ratio": gr / f, "grad": g.cpu().numpy().tolist(),
                    "loglik_rel_diff": float(abs((ph[0] + ph[1]) - (pfh[0] + pfh[1])) / abs(pfh[0] + pfh[1]))})
    print(json.dumps({"tool": "bench_grad", "n": a.n, "kind": a.kind, "theta": a.theta, "launches": a.launches,
                      "rounds": a.rounds, "warmup": a.warmup, "results": out}))


if __name__ == "__main__":
    main()
