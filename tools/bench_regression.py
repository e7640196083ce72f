"""Whitened Gram sweep: timing at BASELINE config 3's size (N = 1e6, m = 15, exponential, Z-ordered) or at --n.
One GPU, one process, synthetic data as bench.py (uniform coordinates, standard-normal values, seed 0).

For ncol = 2, 4, 8, 16 columns, in alternating rounds (--rounds samples per quantity, each `reps` back-to-back calls
after `warmup`, device events around them; medians reported, with min and max):
  * ms per nngp_whiten_gram alone (U and the Gram matrix) on the stored B, F and sorted neighbour rows, and per
    whitening alone (gram = NULL: the first of the three kernels); their difference is the Gram tile kernel plus the
    one-block fold ("gram_part_ms", derived, not timed on its own: the C ABI has no Gram-only call);
  * ms per B/F-writing nngp_bf_sweep followed by nngp_whiten_gram: one likelihood evaluation with ncol - 1 covariates;
  * ms per ncol residual-output sweeps (values and R= given, B and F written: what profile_loglik(mean="constant")
    runs twice), the route the regression would take without the new call.
Also the bytes nngp_whiten_gram must move (B, nbr, F, V gathered once, U written and read again, the tile records)
and the rate that implies at the measured time.  Prints one JSON line; --out writes it to a file as well.
    python tools/bench_regression.py [--n 1000000 --m 15 --rounds 5] [--out profiles/regression/bench_whiten.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth  # noqa: E402
from pynngp_amd import _lib  # noqa: E402
from tools.bench_latent import timed  # noqa: E402


def stats(xs):
    return {"median": sorted(xs)[len(xs) // 2], "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=15)
    ap.add_argument("--phi", type=float, default=30.0)
    ap.add_argument("--tau2", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    coords, y = synth(args.n, 0)
    c = torch.as_tensor(coords).to(dev)
    v = torch.as_tensor(y).to(dev)
    n, m = c.shape[0], args.m
    kind, theta = "exponential", (1.0, args.phi, args.tau2)
    nbr = _lib.knn_prior(c, m)
    order, nbr_sorted = _lib.row_order(c, nbr=nbr)
    del nbr
    lib = _lib.load()
    ws_s = _lib._workspace(lib.nngp_bf_sweep_workspace_bytes(n, m, 0, c.shape[1], 0), dev)
    ws_s.zero_()
    B = torch.empty((n, m), dtype=torch.float64, device=dev)
    F = torch.empty(n, dtype=torch.float64, device=dev)
    R = torch.empty(n, dtype=torch.float64, device=dev)
    part = torch.empty(4, dtype=torch.float64, device=dev)

    def sweep_bf():
        _lib.bf_sweep(c, nbr_sorted, 0, kind, *theta, B=B, F=F, partials=part, workspace=ws_s, order=order)

    def sweep_resid():
        _lib.bf_sweep(c, nbr_sorted, 0, kind, *theta, values=v, B=B, F=F, R=R, partials=part, workspace=ws_s,
                      order=order)

    sweep_bf()
    res = {"tool": "bench_regression", "device": torch.cuda.get_device_name(0), "n": n, "m": m, "kind": kind,
           "theta": theta, "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup, "ncol": {}}
    gen = torch.Generator(dev).manual_seed(1)
    for k in (2, 4, 8, 16):
        V = torch.randn((n, k), dtype=torch.float64, device=dev, generator=gen)
        V[:, 0] = v
        U = torch.empty_like(V)
        ws = _lib._workspace(lib.nngp_whiten_gram_workspace_bytes(n, k), dev)

        def whiten():
            _lib.whiten_gram(nbr_sorted, B, F, V, 0, order=order, U=U, workspace=ws)

        def whiten_only():
            _lib.whiten_gram(nbr_sorted, B, F, V, 0, order=order, U=U, workspace=ws, want_gram=False)

        def sweep_whiten():
            sweep_bf()
            whiten()

        def resid_sweeps():
            for _ in range(k):
                sweep_resid()

        fns = {"whiten_gram": whiten, "whiten_only": whiten_only, "sweep_plus_whiten_gram": sweep_whiten, "ncol_residual_sweeps": resid_sweeps}
        ms = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                ms[name].append(timed(fn, args.warmup, args.reps))
        out = {name: stats(x) for name, x in ms.items()}
        tiles = (n + 1023) // 1024
        # B, nbr, F and order read once; V: its own row and (cache permitting) each row once; U written, then read
        algo_bytes = n * m * (8 + 4) + n * (8 + 4) + 3 * n * k * 8 + 2 * tiles * (k * (k + 1) // 2) * 8
        gather_bytes = n * m * k * 8  # what the gather requests from the caches (V rows re-read per neighbour)
        t = out["whiten_gram"]["median"]
        out.update(gram_part_ms=t - out["whiten_only"]["median"], algorithmic_bytes=algo_bytes, gathered_bytes=gather_bytes,
                   algorithmic_tb_per_s=algo_bytes / (t * 1e-3) / 1e12,
                   gathered_tb_per_s=gather_bytes / (t * 1e-3) / 1e12,
                   ratio_sweeps_over_sweep_plus_whiten=out["ncol_residual_sweeps"]["median"]
                   / out["sweep_plus_whiten_gram"]["median"])
        res["ncol"][str(k)] = out
        del V, U, ws
    res["bf_sweep_ms"] = stats([timed(sweep_bf, args.warmup, args.reps) for _ in range(args.rounds)])
    res["residual_sweep_ms"] = stats([timed(sweep_resid, args.warmup, args.reps) for _ in range(args.rounds)])

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
