#!/usr/bin/env python3
"""Time the packed-row multivariate gradient sweep nngp_bf_grad_mv_obs beside the sweeps it replaces, in one process
(tools/bench_mv.py's protocol and model: N = 1e6 points in 2-D, exponential, untimed launches of each candidate first,
event-bracketed rounds that alternate the candidates of the same build; medians, minima and maxima).

(a) Full mask at (q, m) = (2, 15), (2, 31), (3, 20), (4, 15): the gradient sweep, nngp_bf_sweep_mv_obs likelihood-only
    and with B written, and nngp_bf_grad_mv (the unpacked gradient sweep) in the same rounds.
(b) tools/bench_mv_obs.py's sparse case: q = 2, the second outcome at every fourth site, m = 31 and m = 50, sets cut to
    the longest prefix of slots with at most 64 observed rows.
A central-difference gradient (today's fit() on such data) costs 2 P likelihood-only sweeps, P = q (q + 1) / 2 + 2 q;
that figure is the measured likelihood-only time scaled by 2 P.  Prints one JSON line and writes it to
profiles/mv/bench_mv_obs_grad.json."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pynngp_amd import _lib  # noqa: E402
from tools.bench_mv import AFULL  # noqa: E402
from tools.bench_mv_obs import rounds, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv", "bench_mv_obs_grad.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mv_obs_grad needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    lib = _lib.load()
    kind = "exponential"
    coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, 2))).to(dev)

    def run(q, m, nbr, obs, Y, rows_max, unpacked):
        A, phi, tau2 = AFULL[:q, :q], 30.0 + 25.0 * np.arange(q), 0.05 * (1 + np.arange(q))
        npar = q * (q + 1) // 2 + 2 * q
        ws = _lib._workspace(max(lib.nngp_bf_grad_mv_obs_workspace_bytes(a.n, m, q),
                                 lib.nngp_bf_grad_mv_workspace_bytes(a.n, m, q)), dev)
        grad = lambda: _lib.bf_grad_mv_obs(coords, nbr, 0, kind, A, phi, tau2, obs, rows_max, Y, workspace=ws)
        ob = lambda b: _lib.bf_sweep_mv_obs(coords, nbr, 0, kind, A, phi, tau2, obs, rows_max, Y, want_b=b, want_lf=b,
                                            workspace=ws)
        cands = {"grad": grad, "obs": lambda: ob(False), "obs_b": lambda: ob(True)}
        if unpacked:
            cands["grad_mv"] = lambda: _lib.bf_grad_mv(coords, nbr, 0, kind, A, phi, tau2, Y, workspace=ws)
        s = stats(rounds(cands, a))
        pg, pl = grad()[0].cpu().numpy(), ob(False)[3].cpu().numpy()
        row = {"q": q, "m": m, "rows_max": rows_max, "n_params": npar, **s,
               "grad_over_obs_b": s["grad_ms"] / s["obs_b_ms"], "grad_over_obs": s["grad_ms"] / s["obs_ms"],
               "central_differences_ms": 2 * npar * s["obs_ms"],
               "central_differences_over_grad": 2 * npar * s["obs_ms"] / s["grad_ms"],
               "loglik_terms_rel_diff_grad_vs_obs": abs((pg[0] + pg[1]) - (pl[0] + pl[1])) / abs(pl[0] + pl[1]),
               "flags": [float(pg[2]), float(pg[3])]}
        if unpacked:
            row["packed_over_unpacked"] = s["grad_ms"] / s["grad_mv_ms"]
        print(json.dumps(row), flush=True)
        return row

    full, sparse = [], []
    for q, m in ((2, 15), (2, 31), (3, 20), (4, 15)):
        Y = torch.from_numpy(rng.standard_normal((a.n, q, 1))).to(dev)
        obs = torch.full((a.n,), 2 ** q - 1, dtype=torch.uint8, device=dev)
        full.append(run(q, m, _lib.knn_prior(coords, m), obs, Y, m * q, True))

    q = 2
    obs = (1 + 2 * (torch.arange(a.n, device=dev) % 4 == 0)).to(torch.uint8)
    bits = ((obs[:, None] >> torch.arange(q, device=dev)) & 1) != 0
    Y = torch.from_numpy(rng.standard_normal((a.n, q, 1))).to(dev)
    Y[~bits] = float("nan")
    for m in (31, 50):
        nbr = _lib.knn_prior(coords, m)
        keep = (bits.sum(1)[nbr.long().clamp(min=0)] * (nbr >= 0)).cumsum(1) <= _lib.MV_MAX_ROWS
        nbr = torch.where(keep, nbr, torch.full_like(nbr, -1)).contiguous()
        rows = _lib.mv_obs_rows(nbr, obs)
        row = run(q, m, nbr, obs, Y, int(rows.max()), False)
        sparse.append({**row, "rows_mean": float(rows.double().mean())})

    res = {"tool": "bench_mv_obs_grad", "n": a.n, "kind": kind, "launches": a.launches, "rounds": a.rounds,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "full_mask": full, "sparse": sparse}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
