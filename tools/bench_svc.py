#!/usr/bin/env python3
"""Time the spatially-varying-coefficient sweeps (nngp_bf_sweep_svc, nngp_bf_grad_svc), log-likelihood only, for
r = 1, 2, 4 components in one process against two yardsticks of the same build on the same points and sets:
  (a) nngp_bf_sweep_noise / nngp_bf_grad_noise at v = 1 (isotropic exponential): the same lane-group layout with one
      covariance evaluation per pair; at r = 1, Z = 1 it is the same model;
  (b) the only earlier route to the model: the joint blocks built in torch (nngp_joint_dist, the covariates gathered per
      slot) and factorised by nngp_bf_sweep_blocks.  It materialises (m + 1)(m + 2) / 2 doubles per location, so it is
      timed on the first --blocks-rows locations and scaled by n / blocks_rows (recorded as such).
Warm clocks, untimed launches of each first, event-bracketed rounds that alternate the candidates; medians and minima.
Prints one JSON line and writes it to profiles/svc/bench_svc.json.
python tools/bench_svc.py [--n 1000000] [--m 15 20] [--r 1 2 4]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pynngp_amd import _lib  # noqa: E402

SIGMA2 = (1.0, 0.7, 0.5, 0.4)
PHI = (30.0, 20.0, 45.0, 25.0)


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
    ap.add_argument("--r", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--tau2", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--blocks-rows", type=int, default=100_000)
    ap.add_argument("--blocks-launches", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svc", "bench_svc.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_svc needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, 2))).to(dev)
    y = torch.from_numpy(rng.standard_normal(a.n)).to(dev)
    Zall = torch.from_numpy(np.concatenate([np.ones((a.n, 1)), rng.standard_normal((a.n, 3))], axis=1)).to(dev)
    one = torch.ones(a.n, dtype=torch.float64, device=dev)
    kind, t2 = "exponential", a.tau2
    sub = min(a.blocks_rows, a.n)
    lib = _lib.load()
    out = []
    for m in a.m:
        nbr = _lib.knn_prior(coords, m)
        order, nbs = _lib.row_order(coords, 0, a.n, nbr)
        wsn = _lib._workspace(lib.nngp_bf_sweep_noise_workspace_bytes(a.n, m), dev)
        wsg = _lib._workspace(lib.nngp_bf_grad_workspace_bytes(a.n, m), dev)
        wsb = _lib._workspace(lib.nngp_bf_sweep_blocks_workspace_bytes(sub), dev)
        pb = torch.empty(4, dtype=torch.float64, device=dev)
        nsub = nbr[:sub].contiguous()
        ia, ib = np.tril_indices(m + 1)  # entry a (a + 1) / 2 + b of joint_dist's layout
        ia, ib = torch.from_numpy(ia).to(dev), torch.from_numpy(ib).to(dev)
        diag = (ia == ib)[:, None]

        def noise():
            return _lib.bf_sweep_noise(coords, nbs, 0, kind, SIGMA2[0], PHI[0], t2, one, values=y, want_bf=False,
                                       order=order, workspace=wsn)

        def gnoise():
            return _lib.bf_grad_noise(coords, nbs, 0, kind, SIGMA2[0], PHI[0], t2, y, one, order=order, workspace=wsg)

        fns = {"noise": noise, "grad_noise": gnoise}
        blocks = {}
        for r in a.r:
            Z = Zall[:, :r].contiguous()
            s2, ph = SIGMA2[:r], PHI[:r]
            wss = _lib._workspace(lib.nngp_bf_sweep_svc_workspace_bytes(a.n, m, r), dev)

            def svc(Z=Z, s2=s2, ph=ph, wss=wss):
                return _lib.bf_sweep_svc(coords, Z, nbs, 0, kind, s2, ph, t2, values=y, want_bf=False, order=order,
                                         workspace=wss)

            def gsvc(Z=Z, s2=s2, ph=ph, wss=wss):
                return _lib.bf_grad_svc(coords, Z, nbs, 0, kind, s2, ph, t2, y, order=order, workspace=wss)

            def blk(Z=Z, s2=s2, ph=ph, r=r):
                d = _lib.joint_dist(coords, nsub, 0)  # (ne, sub): 0 on the diagonal, +inf for slots without a point
                idx = torch.cat([nsub.long().clamp(min=0), torch.arange(sub, device=dev)[:, None]], dim=1)
                zf = Z[idx] * torch.cat([nsub >= 0, torch.ones_like(nsub[:, :1], dtype=torch.bool)], dim=1)[..., None]
                cov = t2 * diag.to(torch.float64).expand(-1, sub).clone()
                for k in range(r):
                    cov += (s2[k] * zf[:, ia, k] * zf[:, ib, k]).T * torch.exp(-ph[k] * d)
                return _lib.bf_sweep_blocks(cov, nsub, a.n, 0, values=y, qvalues=y, want_bf=False, workspace=wsb,
                                            partials=pb)

            fns[f"svc_r{r}"], fns[f"grad_svc_r{r}"], blocks[f"blocks_r{r}"] = svc, gsvc, blk
        for fn in fns.values():
            time_ms(fn, a.warmup)
        for fn in blocks.values():
            time_ms(fn, 2)
        t = {k: [] for k in list(fns) + list(blocks)}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                t[k].append(time_ms(fn, a.launches))
            for k, fn in blocks.items():
                t[k].append(time_ms(fn, a.blocks_launches) * (a.n / sub))
        med = {k: float(np.median(x)) for k, x in t.items()}
        row = {"m": m, **{k + "_ms": x for k, x in med.items()}, **{k + "_ms_min": min(x) for k, x in t.items()},
               **{k + "_ms_max": max(x) for k, x in t.items()}}
        for r in a.r:
            row[f"svc_r{r}_over_noise"] = med[f"svc_r{r}"] / med["noise"]
            row[f"grad_svc_r{r}_over_grad_noise"] = med[f"grad_svc_r{r}"] / med["grad_noise"]
            row[f"blocks_r{r}_over_svc"] = med[f"blocks_r{r}"] / med[f"svc_r{r}"]
        # the same answers: r = 1, Z = 1 against the noise sweep, and the blocks route on its rows
        p1, pn = fns[f"svc_r{a.r[0]}"]()[3].cpu().numpy(), noise()[3].cpu().numpy()
        if a.r[0] == 1:
            row["loglik_rel_diff_r1_vs_noise"] = float(abs((p1[0] + p1[1]) - (pn[0] + pn[1])) / abs(pn[0] + pn[1]))
        out.append(row)
    res = {"tool": "bench_svc", "n": a.n, "kind": kind, "sigma2": SIGMA2, "phi": PHI, "tau2": t2, "launches": a.launches,
           "rounds": a.rounds, "warmup": a.warmup, "blocks_rows": sub, "blocks_scaled_by": a.n / sub,
           "device": torch.cuda.get_device_name(0), "results": out}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
