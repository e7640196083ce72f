#!/usr/bin/env python3
"""Time the packed-row multivariate sweep nngp_bf_sweep_mv_obs in one process (tools/bench_mv.py's protocol and model:
N = 1e6 points in 2-D, exponential, untimed launches of each candidate first, event-bracketed rounds that alternate the
candidates; medians, minima and maxima).

(a) Full mask at (q, m) = (2, 15), (2, 31), (3, 20), (4, 15): the new sweep against nngp_bf_sweep_mv of the same build
    in the same rounds, likelihood-only and with B written: the price of packing.
(b) Sparse outcomes: q = 2, the second outcome at every fourth site, m = 31 and m = 50, sets cut to the longest prefix of
    slots with at most 64 observed rows.  Beside it the only other route to this model: dense joint blocks in torch
    (tools/bench_mv.py's route with the rows that are not observed decoupled: unit diagonal, zero value), on
    --torch-rows rows, scaled to N.
Prints one JSON line and writes it to profiles/mv/bench_mv_obs.json."""
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


def torch_route(coords, nbr, Y, bits, A, phi, tau2, lo, hi, chunk):
    """(sum 2 log diag LF, sum |E|^2) over rows [lo, hi) from dense joint Cholesky factors of all (m + 1) q rows, a row
    that is not observed (or a slot without a point) replaced by a decoupled unit row with value 0."""
    q = A.shape[0]
    outer = torch.stack([torch.outer(A[:, k], A[:, k]) for k in range(q)])
    ld = torch.zeros((), dtype=torch.float64, device=coords.device)
    qd = torch.zeros_like(ld)
    for a in range(lo, hi, chunk):
        b = min(a + chunk, hi)
        idx = nbr[a:b].long().clamp(min=0)
        pts = torch.cat([coords[idx], coords[a:b, None]], 1)
        t = pts[:, :, None, :] - pts[:, None, :, :]
        d = torch.sqrt((t * t).sum(-1))
        n = pts.shape[1] * q
        M = torch.cat([bits[idx] & (nbr[a:b] >= 0)[:, :, None], bits[a:b, None]], 1).reshape(b - a, n).double()
        C = sum(torch.exp(-phi[k] * d)[:, :, None, :, None] * outer[k][None, None, :, None, :] for k in range(q))
        C = C.reshape(b - a, n, n) + torch.diag(tau2.repeat(pts.shape[1]))
        C = C * (M[:, :, None] * M[:, None, :]) + torch.diag_embed(1.0 - M)
        L = torch.linalg.cholesky(C)
        y = torch.nan_to_num(torch.cat([Y[idx], Y[a:b, None]], 1).reshape(b - a, n)) * M
        z = torch.linalg.solve_triangular(L, y[:, :, None], upper=False)
        ld += 2.0 * torch.log(torch.diagonal(L, dim1=1, dim2=2)[:, -q:]).sum()
        qd += (z[:, -q:, 0] ** 2).sum()
    return ld, qd


def rounds(cands, a):
    for fn in cands.values():
        time_ms(fn, a.warmup)
    t = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, fn in cands.items():
            t[k].append(time_ms(fn, a.launches))
    return t


def stats(t):
    return {**{k + "_ms": float(np.median(x)) for k, x in t.items()}, **{k + "_ms_min": min(x) for k, x in t.items()},
            **{k + "_ms_max": max(x) for k, x in t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch-rows", type=int, default=131072)
    ap.add_argument("--torch-chunk", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv", "bench_mv_obs.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mv_obs needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    lib = _lib.load()
    kind = "exponential"
    coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, 2))).to(dev)
    full, sparse = [], []

    def model(q):
        return AFULL[:q, :q], 30.0 + 25.0 * np.arange(q), 0.05 * (1 + np.arange(q))

    for q, m in ((2, 15), (2, 31), (3, 20), (4, 15)):
        A, phi, tau2 = model(q)
        Y = torch.from_numpy(rng.standard_normal((a.n, q, 1))).to(dev)
        nbr = _lib.knn_prior(coords, m)
        obs = torch.full((a.n,), 2 ** q - 1, dtype=torch.uint8, device=dev)
        ws = _lib._workspace(lib.nngp_bf_sweep_mv_obs_workspace_bytes(a.n, m, q), dev)
        mv = lambda b: _lib.bf_sweep_mv(coords, nbr, 0, kind, A, phi, tau2, Y, want_b=b, want_lf=b, workspace=ws)
        ob = lambda b: _lib.bf_sweep_mv_obs(coords, nbr, 0, kind, A, phi, tau2, obs, m * q, Y, want_b=b, want_lf=b,
                                            workspace=ws)
        t = rounds({"mv": lambda: mv(False), "obs": lambda: ob(False), "mv_b": lambda: mv(True),
                    "obs_b": lambda: ob(True)}, a)
        s = stats(t)
        p0, p1 = mv(False)[3].cpu().numpy(), ob(False)[3].cpu().numpy()
        row = {"q": q, "m": m, "rows_max": m * q, **s, "obs_over_mv": s["obs_ms"] / s["mv_ms"],
               "obs_b_over_mv_b": s["obs_b_ms"] / s["mv_b_ms"],
               "loglik_terms_rel_diff_obs_vs_mv": abs((p1[0] + p1[1]) - (p0[0] + p0[1])) / abs(p0[0] + p0[1]),
               "flags": [float(p1[2]), float(p1[3])]}
        full.append(row)
        print(json.dumps(row), flush=True)

    q = 2
    A, phi, tau2 = model(q)
    At, pt, tt = (torch.tensor(x, dtype=torch.float64, device=dev) for x in (A, phi, tau2))
    obs = (1 + 2 * (torch.arange(a.n, device=dev) % 4 == 0)).to(torch.uint8)
    bits = ((obs[:, None] >> torch.arange(q, device=dev)) & 1) != 0
    Y = torch.from_numpy(rng.standard_normal((a.n, q, 1))).to(dev)
    Y[~bits] = float("nan")
    lo, hi = 64, min(a.n, 64 + a.torch_rows)
    for m in (31, 50):
        nbr = _lib.knn_prior(coords, m)
        pop = bits.sum(1)[nbr.long().clamp(min=0)] * (nbr >= 0)
        keep = pop.cumsum(1) <= _lib.MV_MAX_ROWS
        n_cut = int((~keep & (nbr >= 0)).any(1).sum())
        nbr = torch.where(keep, nbr, torch.full_like(nbr, -1)).contiguous()
        rows = _lib.mv_obs_rows(nbr, obs)
        rows_max = int(rows.max())
        ws = _lib._workspace(lib.nngp_bf_sweep_mv_obs_workspace_bytes(a.n, m, q), dev)
        ob = lambda b: _lib.bf_sweep_mv_obs(coords, nbr, 0, kind, A, phi, tau2, obs, rows_max, Y, want_b=b, want_lf=b,
                                            workspace=ws)
        dense = lambda: torch_route(coords, nbr, Y[:, :, 0], bits, At, pt, tt, lo, hi, a.torch_chunk)
        t = rounds({"obs": lambda: ob(False), "obs_b": lambda: ob(True)}, a)
        time_ms(dense, 1)
        t["torch"] = [time_ms(dense, 1) * a.n / (hi - lo) for _ in range(a.rounds)]
        s = stats(t)
        sub = _lib.bf_sweep_mv_obs(coords, nbr[lo:hi].contiguous(), lo, kind, A, phi, tau2, obs, rows_max, Y,
                                   want_b=False, want_lf=False)[3].cpu().numpy()
        ld, qd = (float(x) for x in dense())
        ref = next(r for r in full if (r["q"], r["m"]) == (2, 31))
        row = {"q": q, "m": m, "rows_max": rows_max, "rows_mean": float(rows.double().mean()),
               "locations_cut_to_64_rows": n_cut, "torch_rows": hi - lo, **s,
               "obs_over_full_2_31": s["obs_ms"] / ref["obs_ms"], "torch_over_obs": s["torch_ms"] / s["obs_ms"],
               "loglik_terms_rel_diff_obs_vs_torch": abs((sub[0] + sub[1]) - (ld + qd)) / abs(ld + qd),
               "flags": [float(sub[2]), float(sub[3])]}
        sparse.append(row)
        print(json.dumps(row), flush=True)

    res = {"tool": "bench_mv_obs", "n": a.n, "kind": kind, "launches": a.launches, "rounds": a.rounds,
           "warmup": a.warmup, "torch_chunk": a.torch_chunk, "device": torch.cuda.get_device_name(0),
           "full_mask": full, "sparse": sparse}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
