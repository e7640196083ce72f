#!/usr/bin/env python3
"""Time the per-point noise sweeps (nngp_bf_sweep_noise, nngp_bf_grad_noise) in one process against
  1. the homoscedastic forward sweep (nngp_bf_sweep, log-likelihood only) of the same build,
  2. the only other route to the heteroscedastic model: nngp_joint_dist + a torch elementwise covariance with the
     weighted diagonal + nngp_bf_sweep_blocks,
  3. the homoscedastic gradient sweep (nngp_bf_grad).
Warm clocks, >= 200 untimed launches of each first, event-bracketed rounds that alternate the candidates; medians.
Prints one JSON line and writes it to profiles/het/bench_het.json.
python tools/bench_het.py [--n 1000000] [--m 15 20] [--kind exponential]"""
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
    ap.add_argument("--kind", default="exponential")
    ap.add_argument("--theta", type=float, nargs=3, default=[1.0, 30.0, 0.1])
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--blocks-warmup", type=int, default=20, help="untimed runs of the blocks route (ms each)")
    ap.add_argument("--blocks-launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "het", "bench_het.json"))
    a = ap.parse_args()
    if a.kind != "exponential":
        raise SystemExit("the blocks route here evaluates the exponential covariance")
    if not torch.cuda.is_available():
        raise SystemExit("bench_het needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, 2))).to(dev)
    y = torch.from_numpy(rng.standard_normal(a.n)).to(dev)
    v = torch.from_numpy(np.exp(rng.uniform(np.log(0.2), np.log(5.0), a.n)) ** 2).to(dev)
    s2, phi, t2 = a.theta
    lib = _lib.load()
    out = []
    for m in a.m:
        nbr = _lib.knn_prior(coords, m)
        order, nbs = _lib.row_order(coords, 0, a.n, nbr)
        wsf = _lib._workspace(lib.nngp_bf_sweep_workspace_bytes(a.n, m, _lib.KIND_CODES[a.kind], 2, 0), dev)
        wsn = _lib._workspace(lib.nngp_bf_sweep_noise_workspace_bytes(a.n, m), dev)
        wsg = _lib._workspace(lib.nngp_bf_grad_workspace_bytes(a.n, m), dev)
        wsb = _lib._workspace(lib.nngp_bf_sweep_blocks_workspace_bytes(a.n), dev)
        pf = torch.empty(4, dtype=torch.float64, device=dev)
        pb = torch.empty(4, dtype=torch.float64, device=dev)
        dist = torch.empty((int(lib.nngp_joint_entries(m)), a.n), dtype=torch.float64, device=dev)
        diag = _lib.joint_diagonal(m).to(dev)
        # the weight of the point in each diagonal slot of nbr row t (0 where the slot holds none), the location last
        vd = torch.cat([torch.where(nbs >= 0, v[nbs.clamp(min=0).long()], torch.zeros((), dtype=v.dtype, device=dev)).T,
                        v[order.long()][None, :]]) * t2

        def fwd():
            return _lib.bf_sweep(coords, nbs, 0, a.kind, s2, phi, t2, values=y, want_bf=False, partials=pf,
                                 workspace=wsf, order=order)

        def noise():
            return _lib.bf_sweep_noise(coords, nbs, 0, a.kind, s2, phi, t2, v, values=y, want_bf=False, order=order,
                                       workspace=wsn)

        def blocks():
            _lib.joint_dist(coords, nbs, 0, order=order, out=dist)
            c = dist.mul_(-phi).exp_().mul_(s2)
            c[diag] += vd
            return _lib.bf_sweep_blocks(c, nbs, a.n, 0, values=y, qvalues=y, want_bf=False, order=order, workspace=wsb,
                                        partials=pb)

        def grad():
            return _lib.bf_grad(coords, nbs, 0, a.kind, s2, phi, t2, y, order=order, workspace=wsg)

        def gnoise():
            return _lib.bf_grad_noise(coords, nbs, 0, a.kind, s2, phi, t2, y, v, order=order, workspace=wsg)

        for fn in (fwd, noise, grad, gnoise):
            time_ms(fn, a.warmup)
        time_ms(blocks, a.blocks_warmup)
        t = {k: [] for k in ("forward", "noise", "blocks", "grad", "grad_noise")}
        for _ in range(a.rounds):
            t["forward"].append(time_ms(fwd, a.launches))
            t["noise"].append(time_ms(noise, a.launches))
            t["blocks"].append(time_ms(blocks, a.blocks_launches))
            t["grad"].append(time_ms(grad, a.launches))
            t["grad_noise"].append(time_ms(gnoise, a.launches))
        pn = noise()[3].cpu().numpy()
        blocks()
        pbh = pb.cpu().numpy()
        med = {k: float(np.median(x)) for k, x in t.items()}
        out.append({"m": m, **{k + "_ms": x for k, x in med.items()}, **{k + "_ms_min": min(x) for k, x in t.items()},
                    "noise_over_forward": med["noise"] / med["forward"],
                    "blocks_over_noise": med["blocks"] / med["noise"],
                    "grad_noise_over_grad": med["grad_noise"] / med["grad"],
                    "loglik_rel_diff_noise_vs_blocks": float(abs((pn[0] + pn[1]) - (pbh[0] + pbh[1])) /
                                                             abs(pbh[0] + pbh[1]))})
    res = {"tool": "bench_het", "n": a.n, "kind": a.kind, "theta": a.theta, "launches": a.launches, "rounds": a.rounds,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "results": out}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
