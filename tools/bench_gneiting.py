#!/usr/bin/env python3
"""Time the Gneiting space-time sweeps (nngp_bf_sweep_gneiting, nngp_bf_grad_gneiting), log-likelihood only, in one
process against two yardsticks of the same build:
  (a) nngp_bf_sweep_sep / nngp_bf_grad_sep, exponential x exponential, on the same points and sets: the same layout
      with two covariance evaluations per pair where this model makes one plus the time-lag routine;
  (b) the only earlier route to the model: a CallableCovariance with a broadcasting torch callable, its joint blocks
      materialised and factorised by nngp_bf_sweep_blocks.
Warm clocks, untimed launches of each first, event-bracketed rounds that alternate the candidates; medians.
Prints one JSON line and writes it to profiles/gneiting/bench_gneiting.json.
python tools/bench_gneiting.py [--n 1000000] [--m 15 20]"""
import argparse
import json
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, nargs="+", default=[15, 20])
    ap.add_argument("--theta", type=float, nargs=5, default=[1.0, 30.0, 10.0, 0.5, 0.1], help="sigma2 c a beta tau2")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--blocks-warmup", type=int, default=10, help="untimed runs of the callable route (ms each)")
    ap.add_argument("--blocks-launches", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gneiting", "bench_gneiting.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gneiting needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, 3))).to(dev)  # 2-D space + time
    y = torch.from_numpy(rng.standard_normal(a.n)).to(dev)
    s2, c, at, beta, t2 = a.theta
    kind = "exponential"

    def gneiting_matrix(x, z):  # sigma2 exp(-c h psi^(-beta/2)) / psi on (.., ka, 3) x (.., kb, 3) rows: (.., ka, kb)
        d = x[..., :, None, :] - z[..., None, :, :]
        h = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
        psi = 1.0 + (at * d[..., 2]) ** 2
        return s2 * torch.exp(-c * h * psi ** (-0.5 * beta)) / psi

    lib = _lib.load()
    out = []
    for m in a.m:
        scale = torch.tensor([c, c, at], dtype=torch.float64, device=dev)
        nbr = _lib.knn_prior(coords * scale, m)
        order, nbs = _lib.row_order(coords, 0, a.n, nbr)
        wsg = _lib._workspace(lib.nngp_bf_sweep_gneiting_workspace_bytes(a.n, m), dev)
        wss = _lib._workspace(lib.nngp_bf_sweep_sep_workspace_bytes(a.n, m), dev)
        wsb = _lib._workspace(lib.nngp_bf_sweep_blocks_workspace_bytes(a.n), dev)
        pb = torch.empty(4, dtype=torch.float64, device=dev)
        cv = CallableCovariance(gneiting_matrix, tau2=t2)

        def gn():
            return _lib.bf_sweep_gneiting(coords, nbs, 0, kind, s2, c, at, beta, t2, values=y, want_bf=False,
                                          order=order, workspace=wsg)

        def sep():
            return _lib.bf_sweep_sep(coords, nbs, 0, kind, kind, s2, c, at, t2, values=y, want_bf=False, order=order,
                                     workspace=wss)

        def ggn():
            return _lib.bf_grad_gneiting(coords, nbs, 0, kind, s2, c, at, beta, t2, y, order=order, workspace=wsg)

        def gsep():
            return _lib.bf_grad_sep(coords, nbs, 0, kind, kind, s2, c, at, t2, y, order=order, workspace=wss)

        def blocks():
            blk = cv.blocks(coords, nbs, 0, order=order)
            return _lib.bf_sweep_blocks(blk, nbs, a.n, 0, values=y, qvalues=y, want_bf=False, order=order, workspace=wsb,
                                        partials=pb)

        for fn in (gn, sep, ggn, gsep):
            time_ms(fn, a.warmup)
        time_ms(blocks, a.blocks_warmup)
        t = {k: [] for k in ("gneiting", "sep", "blocks", "grad_gneiting", "grad_sep")}
        for _ in range(a.rounds):
            t["gneiting"].append(time_ms(gn, a.launches))
            t["sep"].append(time_ms(sep, a.launches))
            t["blocks"].append(time_ms(blocks, a.blocks_launches))
            t["grad_gneiting"].append(time_ms(ggn, a.launches))
            t["grad_sep"].append(time_ms(gsep, a.launches))
        pg = gn()[3].cpu().numpy()
        blocks()
        pbh = pb.cpu().numpy()
        med = {k: float(np.median(x)) for k, x in t.items()}
        out.append({"m": m, **{k + "_ms": x for k, x in med.items()}, **{k + "_ms_min": min(x) for k, x in t.items()},
                    "gneiting_over_sep": med["gneiting"] / med["sep"],
                    "blocks_over_gneiting": med["blocks"] / med["gneiting"],
                    "grad_gneiting_over_grad_sep": med["grad_gneiting"] / med["grad_sep"],
                    "callable_mode": cv.mode,
                    "loglik_rel_diff_gneiting_vs_blocks": float(abs((pg[0] + pg[1]) - (pbh[0] + pbh[1])) /
                                                                abs(pbh[0] + pbh[1]))})
    res = {"tool": "bench_gneiting", "n": a.n, "kind": kind, "theta": a.theta, "launches": a.launches,
           "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "results": out}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
