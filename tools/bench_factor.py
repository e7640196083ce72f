#!/usr/bin/env python3
"""Times the level-scheduled solves with the NNGP factor (pynngp_amd.NNGPFactor) at config 3's size and writes
profiles/factor/bench_factor.json: the depth of both schedules, wide levels / narrow runs and launch counts, ms
per forward solve, transposed solve and cov_apply at nrhs = 1 and 8, ms per 8 prior draws, a fuse_width sweep, and
beside them precision_apply on the same box -- for uniform random points in input order and for the same points
sorted by x.

Timing: clocks warmed by untimed runs, each sample bracketed by events on the stream, the median over --repeats
samples of --inner back-to-back calls.

    python tools/bench_factor.py [--n 1000000] [--m 15] [--out profiles/factor/bench_factor.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, repeats, inner, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return float(np.median(out))


def measure(coords, args, dev, label):
    from pynngp_amd import Covariance, NNGPFactor, _lib
    from pynngp_amd.factor import DEFAULT_FUSE_WIDTH

    t0 = time.perf_counter()
    f = NNGPFactor(coords, Covariance("exponential", 1.0, args.phi), m=args.m, device=dev)
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    _lib.factor_levels(f.nbr.cpu().numpy(), False)
    levels_s = time.perf_counter() - t0
    n = f.n_nodes
    rng = np.random.default_rng(1)
    V = {k: torch.from_numpy(rng.standard_normal((n, k))).to(dev) for k in (1, 8)}
    rec = {"input": label, "n": n, "m": args.m, "depth": f.depth, "depth_t": f.depth_t,
           "levels_below_64_rows": int((np.diff(f.sched.level_off) < 64).sum()),
           "levels_below_64_rows_t": int((np.diff(f.sched_t.level_off) < 64).sum()),
           "widest_level": int(np.diff(f.sched.level_off).max()), "construct_s": build_s,
           "level_schedule_host_s": levels_s, "default_fuse_width": DEFAULT_FUSE_WIDTH}
    rep, inner = args.repeats, args.inner
    sweep = []
    for w in args.fuse:
        f.fuse_width = w
        row = {"fuse_width": w, **f.n_launches}
        row["forward_ms_nrhs1"] = timed(lambda: f.solve(V[1]), rep, inner)
        row["transposed_ms_nrhs1"] = timed(lambda: f.solve(V[1], trans=True), rep, inner)
        row["forward_ms_nrhs8"] = timed(lambda: f.solve(V[8]), rep, inner)
        sweep.append(row)
        print(label, row, flush=True)
    rec["fuse_width_sweep"] = sweep
    f.fuse_width = DEFAULT_FUSE_WIDTH
    rec["launches"] = f.n_launches
    for k in (1, 8):
        rec[f"forward_ms_nrhs{k}"] = timed(lambda: f.solve(V[k]), rep, inner)
        rec[f"transposed_ms_nrhs{k}"] = timed(lambda: f.solve(V[k], trans=True), rep, inner)
        rec[f"cov_apply_ms_nrhs{k}"] = timed(lambda: f.cov_apply(V[k]), rep, inner)
        rec[f"precision_apply_ms_nrhs{k}"] = timed(lambda: f.precision_apply(V[k]), rep, inner)
    rec["prior_draws_ms_per_8"] = timed(lambda: f._draws(8, 0, None), rep, inner)
    rec["forward_over_precision_apply_nrhs1"] = rec["forward_ms_nrhs1"] / rec["precision_apply_ms_nrhs1"]
    back = f.precision_apply(f.cov_apply(V[8]))
    rec["round_trip_max_abs_err"] = float((back - V[8]).abs().max())
    print(label, {k: v for k, v in rec.items() if k != "fuse_width_sweep"}, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=15)
    ap.add_argument("--phi", type=float, default=30.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--fuse", type=int, nargs="+", default=[0, 16, 64, 256, 1024])
    ap.add_argument("--skip-sorted", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor", "bench_factor.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    coords = np.random.default_rng(0).uniform(0.0, 1.0, (args.n, 2))
    out = {"device": torch.cuda.get_device_name(0), "kind": "exponential", "phi": args.phi,
           "yardstick": "precision_apply_ms_nrhs1 (profiles/latent: 0.236 ms at N = 1e6, m = 15, Z-order storage; "
                        "here the nodes keep their input order)",
           "runs": [measure(coords, args, dev, "uniform random, input order")]}
    if not args.skip_sorted:
        out["runs"].append(measure(coords[np.argsort(coords[:, 0], kind="stable")], args, dev, "sorted by x"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
