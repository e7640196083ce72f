"""Binomial latent posterior (Laplace) timing: N = 1e6, m = 15, exponential, Bernoulli data simulated at theta =
(sigma2, phi) = (1, 17.3) from one exact NNGP draw, intercept-only X.

Measures, on one GPU and in one process:
  * ms per link-kernel launch (nngp_binomial_newton_step with its fold; device events, median of --rounds rounds);
  * BinomialLatentPosterior.mode from a cold start: Newton steps, CG iterations per step with the warm start and,
    from the same cold start, without it, and the wall time of each;
  * the wall time of log_marginal(n_probes = 32) at the mode.
Quotes profiles/gibbs_binomial/bench.json (ms per BinomialSeqNNGP iteration, measured at the parent commit) for scale.
Prints one JSON line and writes it to --out (default profiles/latent/bench_latent_binomial.json).
    python tools/bench_latent_binomial.py [--n 1000000 --m 15 --rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pynngp_amd import BinomialLatentPosterior, Covariance, LatentPosterior, _lib  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def launch_ms(fn, warmup=10, reps=100):
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent", "bench_latent_binomial.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_latent_binomial needs a ROCm GPU (a timing without one says nothing)")
    dev = torch.device("cuda", 0)
    n, m = args.n, args.m
    rng = np.random.default_rng(0)
    coords = rng.uniform(size=(n, 2))
    cov = Covariance("exponential", 1.0, 17.3)
    # the truth: one draw of the NNGP prior (the Gaussian class's sampler with no observation but one)
    y = np.full(n, np.nan)
    y[0] = 0.0
    prior = LatentPosterior(coords, y, cov.replace(tau2=1e6), m=m, device=dev)
    w_true = prior.sample(1, seed=1)[0]
    del prior
    succ = rng.binomial(1, 1.0 / (1.0 + np.exp(-(0.2 + w_true)))).astype(np.float64)
    post = BinomialLatentPosterior(coords, succ, np.ones(n, dtype=np.int64), cov, m=m, X=np.ones((n, 1)), device=dev)

    off = torch.zeros(n, dtype=torch.float64, device=dev)
    bufs = _lib.binomial_newton_step(post.trials, post.successes, off, off, workspace=post._link_ws)
    link = [launch_ms(lambda: _lib.binomial_newton_step(post.trials, post.successes, off, off, *bufs,
                                                        workspace=post._link_ws)) for _ in range(args.rounds)]
    cold = dict(beta0=np.zeros(1), w0=np.zeros(post.n_nodes))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        post.mode(max_newton=1, **cold)  # allocations and first-call costs
        (_, _, cold_info), cold_ms = wall(lambda: post.mode(warm_start=False, **cold))
        (_, _, warm_info), warm_ms = wall(lambda: post.mode(**cold))
    (lm, se), lm_ms = wall(lambda: post.log_marginal(n_probes=32))
    gibbs = json.load(open(os.path.join(ROOT, "profiles", "gibbs_binomial", "bench.json")))
    rec = {
        "workload": f"binomial latent posterior (Laplace), N={n}, m={m}, exponential, Bernoulli data simulated at "
                    "theta=(1, 17.3), intercept-only X, gtol=1e-8, rtol=1e-8",
        "link_kernel_ms": {"rounds": link, "median": statistics.median(link), "max_minus_min": max(link) - min(link)},
        "mode": {"newton_steps": warm_info.newton_steps, "converged": warm_info.converged,
                 "grad_norm": warm_info.grad_norm, "cg_iterations_per_step_warm": list(warm_info.cg_iterations),
                 "wall_ms_warm": warm_ms, "newton_steps_cold_cg": cold_info.newton_steps,
                 "converged_cold_cg": cold_info.converged,
                 "cg_iterations_per_step_cold": list(cold_info.cg_iterations), "wall_ms_cold_cg": cold_ms},
        "log_marginal_32": {"value": lm, "se": se, "wall_ms": lm_ms},
        "gibbs_binomial_iter_ms_parent": gibbs["median"]["binomial_iter_ms"],
        "gibbs_source": "profiles/gibbs_binomial/bench.json",
    }
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
