"""Binomial NNGP sampler timing (N = 1e6, m = 15, exponential, Bernoulli data; 200 iterations after 50 warm-up).

Measures, on one GPU, in one process and in alternating rounds (--rounds of them, every variant once per round):
  * ms per BinomialSeqNNGP iteration (wall clock around `iters` steps, host synchronisations included);
  * ms per Gaussian SeqNNGP iteration on the same field (the empirical logits as the response);
  * the Polya-Gamma launch alone (nngp_gibbs_pg_update, device events) for trials = 1 and trials = 16;
  * the statistics launch alone (nngp_gibbs_pg_stats).
The expectation to report against: a binomial iteration costs no more than a Gaussian one plus the PG launch and
the statistics launch.  Prints one JSON line (median and max - min over the rounds) and writes it to --out
(default profiles/gibbs_binomial/bench.json).
    python tools/bench_gibbs_binomial.py [--n 1000000 --m 15 --iters 200 --warmup 50 --rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pynngp_amd import BinomialSeqNNGP, SeqNNGP, _lib  # noqa: E402


def steps_ms(sampler, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        sampler.step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def launch_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=15)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gibbs_binomial", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gibbs_binomial needs a ROCm GPU (a timing without one says nothing)")
    dev = torch.device("cuda", 0)
    n = args.n
    rng = np.random.default_rng(0)
    coords = rng.uniform(0.0, 1.0, (n, 2))
    eta = -0.3 + 1.2 * np.sin(5.0 * coords[:, 0]) * np.cos(4.0 * coords[:, 1])
    s = rng.binomial(1, 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    trials = np.ones(n, dtype=np.int64)
    kw = dict(m=args.m, kind="exponential", phi=30.0, seed=0, device=dev)
    binom = BinomialSeqNNGP(coords, s, trials, **kw)
    gauss = SeqNNGP(coords, np.log((s + 0.5) / (1.5 - s)), tau2=1.0, **kw)
    t1 = binom.trials
    t16 = torch.full_like(t1, 16)
    kap16 = torch.floor(torch.rand(n, dtype=torch.float64, device=dev) * 17.0) - 8.0
    om, yr, st = torch.empty_like(binom.w), torch.empty_like(binom.w), torch.zeros(1, dtype=torch.int32, device=dev)
    variants = {
        "pg_trials1_ms": lambda: _lib.gibbs_pg_update(t1, binom.kappa, binom.xb, binom.w, 0, 1, omega=om, yres=yr,
                                                      status=st, checked=True),
        "pg_trials16_ms": lambda: _lib.gibbs_pg_update(t16, kap16, binom.xb, binom.w, 0, 1, omega=om, yres=yr,
                                                       status=st, checked=True),
        "pg_stats_ms": lambda: binom._stats_dev(),
    }
    for _ in range(args.warmup):
        binom.step()
        gauss.step()
    rounds = {k: [] for k in ("binomial_iter_ms", "gaussian_iter_ms", *variants)}
    for _ in range(args.rounds):
        rounds["binomial_iter_ms"].append(steps_ms(binom, args.iters))
        rounds["gaussian_iter_ms"].append(steps_ms(gauss, args.iters))
        for k, fn in variants.items():
            rounds[k].append(launch_ms(fn, 10, 100))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    spread = {k: max(v) - min(v) for k, v in rounds.items()}
    budget = med["gaussian_iter_ms"] + med["pg_trials1_ms"] + med["pg_stats_ms"]
    res = {"workload": f"binomial NNGP Gibbs, N={n}, m={args.m}, exponential, Bernoulli data, {args.iters} iterations "
                       f"after {args.warmup} warm-up, {args.rounds} alternating rounds",
           "rounds": rounds, "median": med, "max_minus_min": spread,
           "expectation": {"gaussian_plus_pg_plus_stats_ms": budget, "binomial_iter_ms": med["binomial_iter_ms"],
                           "within": bool(med["binomial_iter_ms"] <= budget)},
           "n_colors": int(binom.n_colors), "phi_accept_rate_binomial": binom.n_accept / max(binom.iteration, 1)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
