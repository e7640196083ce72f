"""Gradient of the latent marginal likelihood: timing at BASELINE config 3's size (N = 1e6, m = 15, exponential) or
at --n.  One GPU, one process, synthetic data as bench.py (uniform coordinates, standard-normal values, seed 0).

Measures, in alternating rounds (--rounds of them, each `reps` launches after `warmup`, device events around the
launches; the spread is max - min over rounds):
  * ms per nngp_bf_dphi sweep (B, F, dB / dphi, dF / dphi) beside nngp_bf_sweep (B, F) and nngp_bf_grad on the same
    coordinates, neighbour sets and Z-order storage;
  * ms per nngp_latent_rows_dot2_batch at 8 columns beside one nngp_precision_ref_apply_batch at 8 columns;
  * wall time of LatentPosterior.log_marginal_grad beside log_marginal at --probes probes (one warm-up call each);
  * with --fit: evaluations and wall time of fit(gradient=True) beside fit() from a start a factor 1.5 off, and
    the log-marginal each ends at.
Prints one JSON line; --out writes it to a file as well.
    python tools/bench_latent_grad.py [--n 1000000 --m 15 --probes 32 --rounds 3] [--fit] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth  # noqa: E402
from pynngp_amd import Covariance, LatentPosterior, _lib  # noqa: E402
from tools.bench_latent import timed, wall_ms  # noqa: E402


def stats(xs):
    return {"median": sorted(xs)[len(xs) // 2], "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=15)
    ap.add_argument("--phi", type=float, default=30.0)
    ap.add_argument("--tau2", type=float, default=0.1)
    ap.add_argument("--probes", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--fit-probes", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    coords, y = synth(args.n, 0)
    cov = Covariance("exponential", 1.0, args.phi, args.tau2)
    lp = LatentPosterior(coords, y, cov, m=args.m, device=dev)
    n, m = lp.n_nodes, lp.m
    res = {"tool": "bench_latent_grad", "device": torch.cuda.get_device_name(0), "n": n, "m": m, "kind": cov.kind,
           "theta": cov.theta, "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup}

    # ---- the sweeps, on the posterior's own storage
    c, nbr = lp.coords, lp.nbr
    B, F = torch.empty_like(lp.B), torch.empty_like(lp.F)
    dB, dF = torch.empty_like(lp.B), torch.empty_like(lp.F)
    ws_s = _lib._workspace(_lib.load().nngp_bf_sweep_workspace_bytes(n, m, 0, c.shape[1], 0), dev)
    ws_s.zero_()
    ws_d = _lib._workspace(_lib.load().nngp_bf_dphi_workspace_bytes(n, m), dev)
    ws_g = _lib._workspace(_lib.load().nngp_bf_grad_workspace_bytes(n, m), dev)
    vals = lp.y
    sweeps = {
        "bf_sweep": lambda: _lib.bf_sweep(c, nbr, 0, cov.kind, 1.0, cov.phi, 0.0, B=B, F=F, workspace=ws_s),
        "bf_dphi": lambda: _lib.bf_dphi(c, nbr, 0, cov.kind, 1.0, cov.phi, 0.0, B=B, F=F, dB=dB, dF=dF, workspace=ws_d),
        "bf_grad": lambda: _lib.bf_grad(c, nbr, 0, cov.kind, *cov.theta, vals, workspace=ws_g),
    }
    X = torch.randn((lp.n_s, 8), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(1))
    out = torch.empty_like(X)
    ws8 = lp._batch_ws(8)
    lp_dB = _lib.bf_dphi(c, nbr, 0, cov.kind, 1.0, cov.phi, 0.0)[2]
    sweeps["rows_dot2_batch_8"] = lambda: _lib.latent_rows_dot2_batch(nbr, lp.B, lp_dB, lp.n_s, X)
    sweeps["precision_ref_apply_batch_8"] = lambda: _lib.precision_ref_apply_batch(*lp._rgeom(), X, d=lp.d, out=out,
                                                                                   workspace=ws8)
    ms = {k: [] for k in sweeps}
    for _ in range(args.rounds):
        for k, fn in sweeps.items():
            ms[k].append(timed(fn, args.warmup, args.reps))
    res["ms_per_launch"] = {k: stats(v) for k, v in ms.items()}

    # ---- the likelihood and its gradient
    kw = dict(n_probes=args.probes, seed=0)
    lp.log_marginal(**kw)
    lp.log_marginal_grad(**kw)
    t_v, t_g = [], []
    for _ in range(args.rounds):
        t_v += wall_ms(lambda: lp.log_marginal(**kw), 1)
        t_g += wall_ms(lambda: lp.log_marginal_grad(**kw), 1)
    value, se, grad, grad_se = lp.log_marginal_grad(**kw)
    res["log_marginal_ms"] = stats(t_v)
    res["log_marginal_grad_ms"] = stats(t_g)
    res["value"], res["se"], res["grad"], res["grad_se"] = value, se, list(map(float, grad)), list(map(float, grad_se))

    if args.fit:
        start = Covariance("exponential", 1.5, args.phi / 1.5, args.tau2 * 1.5)
        fkw = dict(n_probes=args.fit_probes, seed=0)
        fits = {}
        for name, extra in (("nelder_mead", dict(maxiter=60)), ("lbfgsb_gradient", dict(gradient=True, maxiter=15))):
            lp.update(start)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fc, fr = lp.fit(**fkw, **extra)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            ll, lse = lp.log_marginal(**fkw)
            fits[name] = {"nfev": int(fr.nfev), "wall_s": wall, "theta": fc.theta, "log_marginal": ll, "se": lse}
        res["fit"] = fits

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
