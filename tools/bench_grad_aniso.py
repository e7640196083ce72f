#!/usr/bin/env python3
"""Time the per-axis gradient sweep (nngp_bf_grad_aniso) beside the isotropic gradient sweep (nngp_bf_grad) and the
forward log-likelihood sweep (bf_sweep, B / F off) in one process: every shape warmed by untimed launches first, then
event-bracketed rounds that alternate the three sweeps; medians and minima.  The yardstick is nngp_bf_grad on the
same box; beside the ratio stands what the sweep replaces, the 2 (dim + 2) forward sweeps of central differences.
Writes profiles/grad_aniso/bench_grad_aniso.json and prints the same JSON line.
python tools/bench_grad_aniso.py [--n 1000000] [--m 15 20] [--dim 2 3] [--kind exponential]"""
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
    ap.add_argument("--dim", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--kind", default="exponential")
    ap.add_argument("--sigma2", type=float, default=1.0)
    ap.add_argument("--phi", type=float, default=30.0, help="decay of axis 0; axis k has phi * 1.5^k")
    ap.add_argument("--tau2", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_aniso", "bench_grad_aniso.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_aniso needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    out = []
    for dim in a.dim:
        rng = np.random.default_rng(0)
        coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, dim))).to(dev)
        y = torch.from_numpy(rng.standard_normal(a.n)).to(dev)
        phi = tuple(a.phi * 1.5 ** k for k in range(dim))
        scaled = coords * torch.tensor(phi, dtype=torch.float64, device=dev)
        for m in a.m:
            # one neighbour set (the scaled metric's) and one visiting order for all three sweeps
            nbr = _lib.knn_prior(scaled, m)
            order, nbs = _lib.row_order(scaled, 0, a.n, nbr)
            wsf = _lib._workspace(lib.nngp_bf_sweep_workspace_bytes(a.n, m, _lib.KIND_CODES[a.kind], dim, 0), dev)
            wsg = _lib._workspace(lib.nngp_bf_grad_workspace_bytes(a.n, m), dev)
            wsa = _lib._workspace(lib.nngp_bf_grad_aniso_workspace_bytes(a.n, m, dim), dev)
            pf = torch.empty(4, dtype=torch.float64, device=dev)

            def fwd():
                return _lib.bf_sweep(scaled, nbs, 0, a.kind, a.sigma2, 1.0, a.tau2, values=y, want_bf=False,
                                     partials=pf, workspace=wsf, order=order)

            def grad():
                return _lib.bf_grad(scaled, nbs, 0, a.kind, a.sigma2, 1.0, a.tau2, y, order=order, workspace=wsg)

            def aniso():
                return _lib.bf_grad_aniso(coords, nbs, 0, a.kind, a.sigma2, phi, a.tau2, y, order=order,
                                          workspace=wsa)

            for fn in (fwd, grad, aniso):
                time_ms(fn, a.warmup)
            tf, tg, ta = [], [], []
            for _ in range(a.rounds):
                tf.append(time_ms(fwd, a.launches))
                tg.append(time_ms(grad, a.launches))
                ta.append(time_ms(aniso, a.launches))
            pa, ga, _ = aniso()
            pg, gg, _ = grad()
            pa, ga, pg, gg = (t.cpu().numpy() for t in (pa, ga, pg, gg))
            f, g, an = float(np.median(tf)), float(np.median(tg)), float(np.median(ta))
            out.append({"dim": dim, "m": m, "lanes": 2 if m <= 8 else 4 if m <= 15 else 8 if m <= 23 else 16 if m <= 31
                        else 64, "forward_ms": f, "forward_ms_min": min(tf), "grad_ms": g, "grad_ms_min": min(tg),
                        "aniso_ms": an, "aniso_ms_min": min(ta), "aniso_over_grad": an / g,
                        "aniso_over_forward": an / f, "central_difference_forward_sweeps": 2 * (dim + 2),
                        "phi": list(phi), "grad_aniso": ga.tolist(),
                        # Euler's identity against the isotropic sweep at phi = 1 on the scaled coordinates
                        "euler_rel_diff": float(abs(np.dot(phi, ga[1:-1]) - gg[1]) / abs(gg[1])),
                        "loglik_rel_diff": float(abs((pa[0] + pa[1]) - (pg[0] + pg[1])) / abs(pg[0] + pg[1]))})
    res = {"tool": "bench_grad_aniso", "n": a.n, "kind": a.kind, "sigma2": a.sigma2, "tau2": a.tau2,
           "launches": a.launches, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "results": out}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
