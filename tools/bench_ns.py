#!/usr/bin/env python3
"""Time the nonstationary sweep (nngp_bf_sweep_ns, smooth per-point fields) in one process against
  1. the per-point noise sweep (nngp_bf_sweep_noise at v = 1: the same lane-group layout, one scalar theta),
  2. the only other route to the model: nngp_joint_dist + a torch elementwise Paciorek-Schervish covariance from the
     slots' gathered fields + nngp_bf_sweep_blocks.
tools/bench_het.py's protocol: >= 200 untimed launches of each fused candidate first, event-bracketed rounds that
alternate the candidates; medians.  Log-likelihood only (B / F off).  Prints one JSON line and writes it to
profiles/ns/bench_ns.json.
python tools/bench_ns.py [--n 1000000] [--m 15 20]"""
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
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--blocks-warmup", type=int, default=10, help="untimed runs of the blocks route (ms each)")
    ap.add_argument("--blocks-launches", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ns", "bench_ns.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ns needs a GPU")
    dev = torch.device("cuda", 0)
    kind = "exponential"
    rng = np.random.default_rng(0)
    c = rng.uniform(0.0, 1.0, (a.n, 2))
    coords = torch.from_numpy(c).to(dev)
    y = torch.from_numpy(rng.standard_normal(a.n)).to(dev)
    # smooth fields: sigma2 in [0.5, 2], phi in [20, 45], tau2 in [0.05, 0.2]; the scalar theta is their middle
    s2 = torch.from_numpy(0.5 + 1.5 * np.sin(2.0 * c[:, 0] + c[:, 1]) ** 2).to(dev)
    ph = torch.from_numpy(20.0 + 25.0 * (0.5 + 0.5 * np.cos(3.0 * c[:, 1]))).to(dev)
    t2 = torch.from_numpy(0.05 + 0.15 * c[:, 0] ** 2).to(dev)
    one = torch.ones(a.n, dtype=torch.float64, device=dev)
    theta = (1.0, 30.0, 0.1)
    lib = _lib.load()
    out = []
    for m in a.m:
        nbr = _lib.knn_prior(coords, m)
        order, nbs = _lib.row_order(coords, 0, a.n, nbr)
        wsn = _lib._workspace(lib.nngp_bf_sweep_noise_workspace_bytes(a.n, m), dev)
        wss = _lib._workspace(_lib._ns_workspace_bytes(lib, a.n, m, a.n), dev)
        wsb = _lib._workspace(lib.nngp_bf_sweep_blocks_workspace_bytes(a.n), dev)
        pb = torch.empty(4, dtype=torch.float64, device=dev)
        ne = int(lib.nngp_joint_entries(m))
        dist = torch.empty((ne, a.n), dtype=torch.float64, device=dev)
        diag = _lib.joint_diagonal(m).to(dev)
        ia = torch.cat([torch.full((k + 1,), k) for k in range(m + 1)]).to(dev)       # entry e = a (a + 1) / 2 + b
        ib = torch.cat([torch.arange(k + 1) for k in range(m + 1)]).to(dev)
        slot = torch.cat([nbs.T.long(), order.long()[None, :]])                        # (m + 1, n): the point per slot
        has = slot >= 0

        def ns():
            return _lib.bf_sweep_ns(coords, nbs, 0, kind, (s2, ph, t2), values=y, want_bf=False, order=order,
                                    workspace=wss)

        def noise():
            return _lib.bf_sweep_noise(coords, nbs, 0, kind, *theta, one, values=y, want_bf=False, order=order,
                                       workspace=wsn)

        def blocks():
            # per evaluation, as a fit would run it: the slots' fields, then every entry of every block
            sg = torch.where(has, s2[slot.clamp(min=0)], one[:1]).sqrt_()
            pp = torch.where(has, ph[slot.clamp(min=0)], one[:1])
            tt = torch.where(has, t2[slot.clamp(min=0)], one[:1])
            _lib.joint_dist(coords, nbs, 0, order=order, out=dist)
            g = pp[ia] * pp[ib]
            x = 2.0 * g / (pp[ia] ** 2 + pp[ib] ** 2)                                  # d = 2: x^(d/2) = x
            cv = dist.mul_(torch.sqrt(x * g)).neg_().exp_().mul_(x).mul_(sg[ia] * sg[ib])
            cv[diag] = sg * sg + tt
            return _lib.bf_sweep_blocks(cv, nbs, a.n, 0, values=y, qvalues=y, want_bf=False, order=order,
                                        workspace=wsb, partials=pb)

        for fn in (ns, noise):
            time_ms(fn, a.warmup)
        time_ms(blocks, a.blocks_warmup)
        t = {k: [] for k in ("ns", "noise", "blocks")}
        for _ in range(a.rounds):
            t["ns"].append(time_ms(ns, a.launches))
            t["noise"].append(time_ms(noise, a.launches))
            t["blocks"].append(time_ms(blocks, a.blocks_launches))
        pn = ns()[3].cpu().numpy()
        blocks()
        pbh = pb.cpu().numpy()
        med = {k: float(np.median(x)) for k, x in t.items()}
        out.append({"m": m, **{k + "_ms": x for k, x in med.items()}, **{k + "_ms_min": min(x) for k, x in t.items()},
                    "ns_over_noise": med["ns"] / med["noise"], "blocks_over_ns": med["blocks"] / med["ns"],
                    "partials_ns": pn.tolist(),
                    "loglik_rel_diff_ns_vs_blocks": float(abs((pn[0] + pn[1]) - (pbh[0] + pbh[1])) /
                                                          abs(pbh[0] + pbh[1]))})
    res = {"tool": "bench_ns", "n": a.n, "kind": kind, "dim": 2, "theta_noise": theta, "launches": a.launches,
           "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "results": out}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
