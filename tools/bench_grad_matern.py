#!/usr/bin/env python3
"""Time the general-nu Matern gradient sweep (nngp_bf_grad_matern) beside the forward Matern sweep of the same build
(bf_sweep, B / F off) and the Matern-3/2 gradient sweep (nngp_bf_grad) in one process: every shape warmed by untimed
launches first, then event-bracketed rounds that alternate the three sweeps; medians and minima.  The comparison that
matters is against the 2 x 4 forward Matern sweeps of a central difference in four parameters.
Writes profiles/grad_matern/bench_grad_matern.json and prints the same JSON line.
python tools/bench_grad_matern.py [--n 1000000] [--m 15 20] [--nu 1.3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    ap.add_argument("--nu", type=float, default=1.3)
    ap.add_argument("--sigma2", type=float, default=1.0)
    ap.add_argument("--phi", type=float, default=30.0)
    ap.add_argument("--tau2", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_matern", "bench_grad_matern.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_matern needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    rng = np.random.default_rng(0)
    coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, 2))).to(dev)
    y = torch.from_numpy(rng.standard_normal(a.n)).to(dev)
    out = []
    for m in a.m:
        nbr = _lib.knn_prior(coords, m)
        order, nbs = _lib.row_order(coords, 0, a.n, nbr)
        wsf = _lib._workspace(lib.nngp_bf_sweep_workspace_bytes(a.n, m, _lib.KIND_CODES["matern"], 2, 0), dev)
        wsg = _lib._workspace(lib.nngp_bf_grad_workspace_bytes(a.n, m), dev)
        wsm = _lib._workspace(lib.nngp_bf_grad_matern_workspace_bytes(a.n, m), dev)
        pf = torch.empty(4, dtype=torch.float64, device=dev)

        def fwd():
            return _lib.bf_sweep(coords, nbs, 0, "matern", a.sigma2, a.phi, a.tau2, values=y, want_bf=False,
                                 partials=pf, workspace=wsf, order=order, nu=a.nu)

        def grad32():
            return _lib.bf_grad(coords, nbs, 0, "matern32", a.sigma2, a.phi, a.tau2, y, order=order, workspace=wsg)

        def gradm():
            return _lib.bf_grad_matern(coords, nbs, 0, a.sigma2, a.phi, a.tau2, a.nu, y, order=order, workspace=wsm)

        for fn in (fwd, grad32, gradm):
            time_ms(fn, a.warmup)
        tf, tg, tm = [], [], []
        for _ in range(a.rounds):
            tf.append(time_ms(fwd, a.launches))
            tg.append(time_ms(grad32, a.launches))
            tm.append(time_ms(gradm, a.launches))
        pm, gm, _ = gradm()
        fwd()
        pm, gm, pfh = (t.cpu().numpy() for t in (pm, gm, pf))
        f, g, mt = float(np.median(tf)), float(np.median(tg)), float(np.median(tm))
        out.append({"m": m, "lanes": 2 if m <= 8 else 4 if m <= 15 else 8 if m <= 23 else 16 if m <= 31 else 64,
                    "forward_matern_ms": f, "forward_matern_ms_min": min(tf), "grad_matern32_ms": g,
                    "grad_matern32_ms_min": min(tg), "grad_matern_ms": mt, "grad_matern_ms_min": min(tm),
                    "grad_matern_over_forward": mt / f, "grad_matern_over_grad_matern32": mt / g,
                    "central_difference_forward_sweeps": 8, "central_difference_over_grad_matern": 8 * f / mt,
                    "grad": gm.tolist(),
                    "loglik_rel_diff": float(abs((pm[0] + pm[1]) - (pfh[0] + pfh[1])) / abs(pfh[0] + pfh[1]))})
    res = {"tool": "bench_grad_matern", "n": a.n, "dim": 2, "nu": a.nu, "sigma2": a.sigma2, "phi": a.phi,
           "tau2": a.tau2, "launches": a.launches, "rounds": a.rounds, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "results": out}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
