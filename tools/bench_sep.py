#!/usr/bin/env python3
"""Time the separable space-time sweeps (nngp_bf_sweep_sep, nngp_bf_grad_sep), log-likelihood only, in one process
against two yardsticks this change does not touch:
  (a) nngp_bf_sweep_noise / nngp_bf_grad_noise of the same build at v = 1 on the same points (isotropic exponential):
      the same lane-group layout with one covariance evaluation per pair instead of two;
  (b) the only earlier route to the product model: a CallableCovariance with a broadcasting torch callable, its joint
      blocks materialised and factorised by nngp_bf_sweep_blocks.
Warm clocks, untimed launches of each first, event-bracketed rounds that alternate the candidates; medians.
Prints one JSON line and writes it to profiles/sep/bench_sep.json.
python tools/bench_sep.py [--n 1000000] [--m 15 20]"""
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
    ap.add_argument("--theta", type=float, nargs=4, default=[1.0, 30.0, 10.0, 0.1], help="sigma2 phi_s phi_t tau2")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--blocks-warmup", type=int, default=10, help="untimed runs of the callable route (ms each)")
    ap.add_argument("--blocks-launches", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sep", "bench_sep.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sep needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, 3))).to(dev)  # 2-D space + time
    y = torch.from_numpy(rng.standard_normal(a.n)).to(dev)
    one = torch.ones(a.n, dtype=torch.float64, device=dev)
    s2, ps, pt, t2 = a.theta
    kind = "exponential"

    def product_matrix(x, z):  # sigma2 exp(-phi_s |ds| - phi_t |dt|) on (.., ka, 3) x (.., kb, 3) rows: (.., ka, kb)
        d = x[..., :, None, :] - z[..., None, :, :]
        ds = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
        return s2 * torch.exp(-ps * ds - pt * d[..., 2].abs())

    lib = _lib.load()
    out = []
    for m in a.m:
        scale = torch.tensor([ps, ps, pt], dtype=torch.float64, device=dev)
        nbr = _lib.knn_prior(coords * scale, m)
        order, nbs = _lib.row_order(coords, 0, a.n, nbr)
        wss = _lib._workspace(lib.nngp_bf_sweep_sep_workspace_bytes(a.n, m), dev)
        wsn = _lib._workspace(lib.nngp_bf_sweep_noise_workspace_bytes(a.n, m), dev)
        wsg = _lib._workspace(lib.nngp_bf_grad_workspace_bytes(a.n, m), dev)
        wsb = _lib._workspace(lib.nngp_bf_sweep_blocks_workspace_bytes(a.n), dev)
        pb = torch.empty(4, dtype=torch.float64, device=dev)
        cv = CallableCovariance(product_matrix, tau2=t2)

        def sep():
            return _lib.bf_sweep_sep(coords, nbs, 0, kind, kind, s2, ps, pt, t2, values=y, want_bf=False, order=order,
                                     workspace=wss)

        def noise():
            return _lib.bf_sweep_noise(coords, nbs, 0, kind, s2, ps, t2, one, values=y, want_bf=False, order=order,
                                       workspace=wsn)

        def gsep():
            return _lib.bf_grad_sep(coords, nbs, 0, kind, kind, s2, ps, pt, t2, y, order=order, workspace=wss)

        def gnoise():
            return _lib.bf_grad_noise(coords, nbs, 0, kind, s2, ps, t2, y, one, order=order, workspace=wsg)

        def blocks():
            blk = cv.blocks(coords, nbs, 0, order=order)
            return _lib.bf_sweep_blocks(blk, nbs, a.n, 0, values=y, qvalues=y, want_bf=False, order=order, workspace=wsb,
                                        partials=pb)

        for fn in (sep, noise, gsep, gnoise):
            time_ms(fn, a.warmup)
        time_ms(blocks, a.blocks_warmup)
        t = {k: [] for k in ("sep", "noise", "blocks", "grad_sep", "grad_noise")}
        for _ in range(a.rounds):
            t["sep"].append(time_ms(sep, a.launches))
            t["noise"].append(time_ms(noise, a.launches))
            t["blocks"].append(time_ms(blocks, a.blocks_launches))
            t["grad_sep"].append(time_ms(gsep, a.launches))
            t["grad_noise"].append(time_ms(gnoise, a.launches))
        ps_ = sep()[3].cpu().numpy()
        blocks()
        pbh = pb.cpu().numpy()
        med = {k: float(np.median(x)) for k, x in t.items()}
        out.append({"m": m, **{k + "_ms": x for k, x in med.items()}, **{k + "_ms_min": min(x) for k, x in t.items()},
                    "sep_over_noise": med["sep"] / med["noise"],
                    "blocks_over_sep": med["blocks"] / med["sep"],
                    "grad_sep_over_grad_noise": med["grad_sep"] / med["grad_noise"],
                    "callable_mode": cv.mode,
                    "loglik_rel_diff_sep_vs_blocks": float(abs((ps_[0] + ps_[1]) - (pbh[0] + pbh[1])) /
                                                           abs(pbh[0] + pbh[1]))})
    res = {"tool": "bench_sep", "n": a.n, "kinds": [kind, kind], "theta": a.theta, "launches": a.launches,
           "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "results": out}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
