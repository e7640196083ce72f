"""Latent-field posterior timing at BASELINE config 3's size (N = 1e6, m = 15, exponential, tau2 / sigma2 = 0.1).

Measures, on one GPU and in one process:
  * ms per application of the precision operator A = (I - B)^T (sigma2 F)^-1 (I - B) + diag(h / tau2)
    (nngp_precision_apply: two gathers, nothing assembled) and its share of the HBM roofline -- bench.py's peak
    constant and algorithmic-bytes convention; bytes counted per location: nbr 4m, B 8m, rev_j 4m, Brev 8m and
    the vectors (row phase: x, invF, t; column phase: off, t, d, x, out);
  * the same operator through stock PyTorch: (I - B) and its transpose as fp64 ``torch.sparse_csr_tensor``s,
    two sparse products plus the diagonal scalings, after the same warm-up and with the same repeat count;
  * the CG iteration count and the wall time of the posterior mean to rtol 1e-8, beside what a Gibbs estimate
    of the same iteration count would cost at --gibbs-ms per sweep.
With --nrhs K1,K2,... it measures the batched operator instead (nngp_precision_apply_batch, vectors (n, nrhs)):
  * ms per batched application at each nrhs beside the single operator, both timed in this process in
    alternating rounds (--rounds of them, each `reps` applications after `warmup`), with the spread over rounds;
  * the wall time of 8 posterior draws through the batched path (LatentPosterior.sample) beside the loop of
    single square-root applications and single solves that served before it, and of marginal_variance(64);
  * the gate: one application at nrhs = 8 against 8 single applications.
With --ref N_S it measures the posterior on a reference set of N_S points drawn uniformly in the data's bounding
box (seed 1), the leaves integrated out (nngp_precision_ref_*, nngp_latent_ref_cg_batch), beside the AUGMENTED system:
the same node DAG (reference points, then every data location as a leaf, d = 0 on a node without data) through
the S = T calls nngp_precision_apply_batch / nngp_latent_cg_batch (the same arithmetic and resource usage as before
the reference-set forms were added).  Both run in this
process in alternating rounds: ms per application, iterations and wall time of the posterior mean to --rtol, 8
draws at every data location, and the solver's workspace bytes; the gate is the mean solve, eliminated against
augmented beyond three times the larger max - min spread of the pair.
With --logdet it measures log det A by stochastic Lanczos quadrature (LatentPosterior.logdet: --probes Rademacher
probes, eight per batched solve with a trace, to --logdet-rtol): the wall time of --rounds calls after one warm-up
call, the iterations per probe, the value and its standard error, and the wall time of log_marginal beside it.
Synthetic data as bench.py (uniform coordinates, standard-normal values, seed 0); prints one JSON line.
    python tools/bench_latent.py [--n 1000000 --m 15 --reps 1000 --warmup 100] [--nrhs 1,2,4,8 --rounds 3]
    python tools/bench_latent.py --ref 100000 [--rounds 3 --reps 200]
    python tools/bench_latent.py --logdet [--probes 32 --rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import HBM_PEAK, synth  # noqa: E402
from pynngp_amd import Covariance, LatentPosterior, _lib  # noqa: E402


def bytes_per_location(m):
    # nbr 4m + B 8m (row phase), rev_j 4m + Brev 8m (column phase), vectors: x, invF, t | off, t, d, x, out
    return 24 * m + 3 * 8 + (4 + 4 * 8)


def timed(fn, warmup, reps):
    """ms per call from device events around `reps` back-to-back calls, after `warmup` calls."""
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


def sample_loop_single(lp, n_draws, seed, rtol):
    """The draws as a loop over single right-hand sides: one square-root application, one CG solve and one
    device-to-host copy per draw (what LatentPosterior.sample did before the batched solver)."""
    import numpy as np

    b = lp._rhs(())
    out = np.empty((n_draws, lp.n))
    z1 = torch.empty(lp.n, dtype=torch.float64, device=lp.device)
    z2 = torch.empty_like(z1)
    for k in range(n_draws):
        _lib.gibbs_normals(z1, seed, 2 * k)
        _lib.gibbs_normals(z2, seed, 2 * k + 1)
        eta = _lib.precision_sqrt_t_apply(*lp._geom(), z1, z2, d=lp.d)
        w, _ = lp._solve(b + eta, rtol, None)
        out[k] = w[lp.pos].cpu().numpy()
    return out


def wall_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def bench_batch(lp, args, res):
    """The --nrhs measurement (see the module docstring); fills res."""
    import numpy as np

    n, m, dev = lp.n, lp.m, lp.device
    geom = lp._geom()
    gen = torch.Generator(dev).manual_seed(1)
    x1 = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    o1 = torch.empty_like(x1)
    ws1 = lp._batch_ws(1)
    variants = {"single": lambda: _lib.precision_apply(*geom, x1, d=lp.d, out=o1, workspace=ws1)}
    for k in args.nrhs:
        xk = torch.randn((n, k), dtype=torch.float64, device=dev, generator=gen)
        ok = torch.empty_like(xk)
        ws = _lib._workspace(_lib.load().nngp_precision_batch_workspace_bytes(n, k), dev)
        variants[f"nrhs{k}"] = (lambda xk=xk, ok=ok, ws=ws:
                                _lib.precision_apply_batch(*geom, xk, d=lp.d, out=ok, workspace=ws))
    rounds = {name: [] for name in variants}
    for r in range(args.rounds):  # alternating: every variant once per round
        for name, fn in variants.items():
            rounds[name].append(timed(fn, args.warmup if r == 0 else 10, args.reps))
    med = {name: statistics.median(v) for name, v in rounds.items()}
    spread = {name: max(v) - min(v) for name, v in rounds.items()}
    res.update(rounds=args.rounds, operator_ms_rounds=rounds, operator_ms_median=med, operator_ms_spread=spread)
    per = {}
    for k in args.nrhs:
        bpc = (24 * m + 60 * k) / k  # algorithmic bytes per location and column
        per[str(k)] = {"ms": med[f"nrhs{k}"], "ms_per_column": med[f"nrhs{k}"] / k,
                       "speedup_per_column_vs_single": med["single"] * k / med[f"nrhs{k}"],
                       "algorithmic_bytes_per_location_and_column": bpc,
                       "hbm_frac": bpc * k * n / (med[f"nrhs{k}"] * 1e-3) / HBM_PEAK}
    res["batched"] = per
    if 8 in args.nrhs:
        margin = 8 * med["single"] - med["nrhs8"]
        worst = 3 * max(8 * spread["single"], spread["nrhs8"])
        res["gate_operator"] = {"eight_single_ms": 8 * med["single"], "one_nrhs8_ms": med["nrhs8"], "margin_ms": margin,
                                "three_times_larger_spread_ms": worst, "passed": bool(margin > worst)}
    # draws: the loop over single right-hand sides against the batched path, alternating; the same bits
    ref = sample_loop_single(lp, 8, 0, args.rtol)
    got = lp.sample(8, seed=0, rtol=args.rtol)
    res["draws_bit_identical"] = bool(np.array_equal(ref, got))
    loop_ms, batch_ms = [], []
    for _ in range(args.rounds):
        loop_ms += wall_ms(lambda: sample_loop_single(lp, 8, 0, args.rtol), 1)
        batch_ms += wall_ms(lambda: lp.sample(8, seed=0, rtol=args.rtol), 1)
    mv_ms = wall_ms(lambda: lp.marginal_variance(64, seed=0, rtol=args.rtol), 2)
    res.update(sample8_single_loop_ms=loop_ms, sample8_batched_ms=batch_ms,
               sample8_speedup=statistics.median(loop_ms) / statistics.median(batch_ms),
               marginal_variance64_ms=mv_ms,
               gate_sample={"passed": bool(statistics.median(batch_ms) <= statistics.median(loop_ms))})


def bench_ref(coords, y, args, dev):
    """The --ref measurement (see the module docstring): the result dict."""
    import numpy as np

    c_host = coords.detach().cpu().numpy() if isinstance(coords, torch.Tensor) else np.asarray(coords)
    lo, hi = c_host.min(axis=0), c_host.max(axis=0)
    ref = np.random.default_rng(1).uniform(lo, hi, (args.ref, c_host.shape[1]))
    cov = Covariance("exponential", args.sigma2, args.phi, args.tau2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lp = LatentPosterior(coords, y, cov, m=args.m, device=dev, ref=ref)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    n, n_s, lib = lp.n_nodes, lp.n_s, _lib.load()
    aug, elim = lp._geom(), lp._rgeom()
    ws_bytes = {"eliminated": {str(k): lib.nngp_latent_ref_cg_batch_workspace_bytes(n, n_s, k) for k in (1, 8)},
                "augmented": {str(k): lib.nngp_latent_cg_batch_workspace_bytes(n, k) for k in (1, 8)}}
    ws_e = _lib._workspace(ws_bytes["eliminated"]["8"], dev)
    ws_a = _lib._workspace(ws_bytes["augmented"]["8"], dev)
    gen = torch.Generator(dev).manual_seed(1)
    xs = torch.randn((n_s, 1), dtype=torch.float64, device=dev, generator=gen)
    xa = torch.randn((n, 1), dtype=torch.float64, device=dev, generator=gen)
    os_, oa = torch.empty_like(xs), torch.empty_like(xa)
    b_s = lp._rhs(())
    b_a = (lp.d * lp.y)[:, None].contiguous()
    max_iter = 20000
    seed = 0

    def mean_elim():
        X, info = _lib.latent_ref_cg_batch(*elim, b_s[:, None].contiguous(), torch.zeros((n_s, 1), dtype=torch.float64,
                                                                                         device=dev),
                                           d=lp.d, rtol=args.rtol, max_iter=max_iter, workspace=ws_e)
        return lp._node_cols(X, lp._leaf_v((), 1)), info

    def mean_aug():
        return _lib.latent_cg_batch(*aug, b_a, torch.zeros_like(b_a), d=lp.d, rtol=args.rtol, max_iter=max_iter,
                                    workspace=ws_a)

    def draws_aug():
        Z1 = torch.empty((n, 8), dtype=torch.float64, device=dev)
        Z2 = torch.empty_like(Z1)
        zz = torch.empty(n, dtype=torch.float64, device=dev)
        for c in range(8):
            Z1[:, c] = _lib.gibbs_normals(zz, seed, 2 * c)
            Z2[:, c] = _lib.gibbs_normals(zz, seed, 2 * c + 1)
        eta = _lib.precision_sqrt_t_apply_batch(*aug, Z1, Z2, d=lp.d, workspace=ws_a)
        R = (b_a + eta).contiguous()
        X, _ = _lib.latent_cg_batch(*aug, R, torch.zeros_like(R), d=lp.d, rtol=args.rtol, max_iter=max_iter,
                                    workspace=ws_a)
        return X[lp.slot_of_t].t().cpu().numpy()

    ops = {"eliminated": lambda: _lib.precision_ref_apply_batch(*elim, xs, d=lp.d, out=os_, workspace=ws_e),
           "augmented": lambda: _lib.precision_apply_batch(*aug, xa, d=lp.d, out=oa, workspace=ws_a)}
    means = {"eliminated": mean_elim, "augmented": mean_aug}
    draws = {"eliminated": lambda: lp.sample(8, seed=seed, rtol=args.rtol), "augmented": draws_aug}
    we, ie = mean_elim()
    wa, ia = mean_aug()  # (both warm now)
    diff = float((we[:, 0] - wa[:, 0]).abs().max() / wa[:, 0].abs().max())
    op_ms = {k: [] for k in ops}
    mean_ms = {k: [] for k in ops}
    draw_ms = {k: [] for k in ops}
    for r in range(args.rounds):  # alternating: every variant once per round
        for k in ops:
            op_ms[k].append(timed(ops[k], args.warmup if r == 0 else 10, args.reps))
        for k in ops:
            mean_ms[k] += wall_ms(means[k], 1)
        for k in ops:
            draw_ms[k] += wall_ms(draws[k], 1)
    med = lambda v: statistics.median(v)  # noqa: E731
    spread = lambda v: max(v) - min(v)  # noqa: E731
    margin = med(mean_ms["augmented"]) - med(mean_ms["eliminated"])
    worst = 3 * max(spread(mean_ms["augmented"]), spread(mean_ms["eliminated"]))
    return {"workload": f"latent posterior on a reference set, N={lp.n} data, n_S={n_s}, nodes={n}, m={args.m}, "
                        f"exponential, sigma2={args.sigma2}, phi={args.phi}, tau2={args.tau2}",
            "setup_s": setup_s, "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup, "rtol": args.rtol,
            "operator_ms_rounds": op_ms, "operator_ms_median": {k: med(v) for k, v in op_ms.items()},
            "mean_iterations": {"eliminated": int(ie[0, 0]), "augmented": int(ia[0, 0])},
            "mean_converged": {"eliminated": bool(ie[0, 1] > 0), "augmented": bool(ia[0, 1] > 0)},
            "mean_wall_ms_rounds": mean_ms, "mean_wall_ms_median": {k: med(v) for k, v in mean_ms.items()},
            "mean_wall_ms_spread": {k: spread(v) for k, v in mean_ms.items()},
            "mean_max_rel_diff_between_variants": diff,
            "sample8_wall_ms_rounds": draw_ms, "sample8_wall_ms_median": {k: med(v) for k, v in draw_ms.items()},
            "cg_workspace_bytes": ws_bytes,
            "cg_workspace_ratio_nrhs1": ws_bytes["eliminated"]["1"] / ws_bytes["augmented"]["1"],
            "gate_mean": {"augmented_minus_eliminated_ms": margin, "three_times_larger_spread_ms": worst,
                          "eliminated_no_slower": bool(margin >= -worst)}}


def bench_logdet(lp, args, res):
    """The --logdet measurement (see the module docstring); fills res."""
    lp.logdet(n_probes=8, seed=1, rtol=args.logdet_rtol)  # warm-up: the workspace and the trace's first allocation
    out = {}

    def run():
        out["ld"] = lp.logdet(n_probes=args.probes, seed=0, rtol=args.logdet_rtol)

    walls = wall_ms(run, args.rounds)
    ld = out["ld"]
    its = [int(v) for v in ld.iterations]

    def run_lm():
        out["lm"] = lp.log_marginal(n_probes=args.probes, seed=0, rtol=args.rtol, logdet_rtol=args.logdet_rtol)

    lm_walls = wall_ms(run_lm, args.rounds)
    res.update(probes=args.probes, logdet_rtol=args.logdet_rtol, rounds=args.rounds, logdet_wall_ms_rounds=walls,
               logdet_wall_ms_median=statistics.median(walls), logdet_wall_ms_spread=max(walls) - min(walls),
               logdet_wall_ms_per_probe=statistics.median(walls) / args.probes, iterations_per_probe=its,
               iterations_min=min(its), iterations_max=max(its), logdet_value=ld.value, logdet_se=ld.se,
               logdet_se_relative=ld.se / abs(ld.value), log_marginal_value=out["lm"][0], log_marginal_se=out["lm"][1],
               log_marginal_wall_ms_rounds=lm_walls, log_marginal_wall_ms_median=statistics.median(lm_walls))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=15)
    ap.add_argument("--sigma2", type=float, default=1.0)
    ap.add_argument("--phi", type=float, default=30.0)
    ap.add_argument("--tau2", type=float, default=0.1)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--gibbs-ms", type=float, default=0.80, help="ms per Gibbs iteration to compare against")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--nrhs", type=lambda v: [int(t) for t in v.split(",")], default=None,
                    help="comma-separated column counts: measure the batched operator and the batched draws instead")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds per variant (--nrhs, --ref)")
    ap.add_argument("--ref", type=int, default=None,
                    help="reference-set size: measure the eliminated system against the augmented one instead")
    ap.add_argument("--logdet", action="store_true",
                    help="measure log det A by stochastic Lanczos quadrature (and log_marginal) instead")
    ap.add_argument("--probes", type=int, default=32, help="probes of the --logdet run")
    ap.add_argument("--logdet-rtol", type=float, default=1e-6, help="tolerance of the probe solves (--logdet)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_latent needs a ROCm GPU (a timing without one says nothing)")
    dev = torch.device("cuda", 0)
    n, m = args.n, args.m
    coords, y = synth(n)
    if args.ref:
        print(json.dumps(bench_ref(coords, y, args, dev)))
        return
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lp = LatentPosterior(coords, y, Covariance("exponential", args.sigma2, args.phi, args.tau2), m=m, device=dev)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0

    if args.logdet:
        res = {"workload": f"latent posterior, log det A by stochastic Lanczos quadrature, N={n}, m={m}, exponential, "
                           f"sigma2={args.sigma2}, phi={args.phi}, tau2={args.tau2}",
               "setup_s": setup_s}
        bench_logdet(lp, args, res)
        print(json.dumps(res))
        return

    if args.nrhs:
        res = {"workload": f"latent posterior, batched operator, N={n}, m={m}, exponential, sigma2={args.sigma2}, "
                           f"phi={args.phi}, tau2={args.tau2}",
               "setup_s": setup_s, "reps": args.reps, "warmup": args.warmup, "hbm_peak_GBps": HBM_PEAK / 1e9}
        bench_batch(lp, args, res)
        print(json.dumps(res))
        return

    geom = lp._geom()
    x = torch.randn(n, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(1))
    out = torch.empty_like(x)
    ws1 = lp._batch_ws(1)
    op_ms = timed(lambda: _lib.precision_apply(*geom, x, d=lp.d, out=out, workspace=ws1), args.warmup, args.reps)
    bpl = bytes_per_location(m)
    res = {"workload": f"latent posterior, N={n}, m={m}, exponential, sigma2={args.sigma2}, phi={args.phi}, "
                       f"tau2={args.tau2}",
           "setup_s": setup_s, "operator_ms": op_ms, "algorithmic_bytes_per_location": bpl,
           "operator_GBps": bpl * n / (op_ms * 1e-3) / 1e9, "hbm_peak_GBps": HBM_PEAK / 1e9,
           "operator_hbm_frac": bpl * n / (op_ms * 1e-3) / HBM_PEAK, "reps": args.reps, "warmup": args.warmup}

    if not args.no_baseline:
        # the same operator through stock PyTorch sparse products (storage order, as the kernel sees it)
        nbr = lp.nbr.long()
        valid = nbr >= 0
        rows = torch.arange(n, device=dev)[:, None].expand(n, m)[valid]
        ii = torch.cat([torch.arange(n, device=dev), rows])
        jj = torch.cat([torch.arange(n, device=dev), nbr[valid]])
        vv = torch.cat([torch.ones(n, dtype=torch.float64, device=dev), -lp.B[valid]])
        IB = torch.sparse_coo_tensor(torch.stack([ii, jj]), vv, (n, n)).coalesce().to_sparse_csr()
        IBt = torch.sparse_coo_tensor(torch.stack([jj, ii]), vv, (n, n)).coalesce().to_sparse_csr()
        scale = (1.0 / (lp.F * args.sigma2)).contiguous()
        x2 = x[:, None].contiguous()

        def stock():
            t = torch.mm(IB, x2)
            t.mul_(scale[:, None])
            o = torch.mm(IBt, t)
            return o.addcmul_(lp.d[:, None], x2)

        ref = stock()[:, 0]  # (a torch build without sparse CSR products on the GPU fails here, loudly)
        _lib.precision_apply(*geom, x, d=lp.d, out=out, workspace=ws1)
        res["baseline_max_rel_diff"] = float(((out - ref).abs().max() / ref.abs().max()).item())
        base_ms = timed(stock, args.warmup, args.reps)
        # alternate once more, to see the spread of both on a shared machine
        op_ms2 = timed(lambda: _lib.precision_apply(*geom, x, d=lp.d, out=out, workspace=ws1), 10, args.reps)
        base_ms2 = timed(stock, 10, args.reps)
        res.update(baseline="torch.sparse_csr_tensor fp64: (I - B) x, scale, (I - B)^T t, + d x",
                   baseline_ms=base_ms, operator_ms_repeat=op_ms2, baseline_ms_repeat=base_ms2,
                   speedup_vs_baseline=base_ms / op_ms)
        del IB, IBt

    # the posterior mean: CG to rtol (b = h y / tau2; no covariates)
    b = lp._rhs(())
    lp._solve(b, args.rtol, None)  # warm-up solve
    walls, iters = [], 0
    for _ in range(args.solves):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info = lp._solve(b, args.rtol, None)
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0))
        iters = info.iterations
    res.update(cg_rtol=args.rtol, cg_iterations=iters, cg_converged=bool(info.converged),
               cg_wall_ms=statistics.median(walls), cg_wall_ms_all=walls,
               cg_ms_per_iteration=statistics.median(walls) / max(iters, 1),
               gibbs_ms_per_iteration=args.gibbs_ms, gibbs_ms_for_as_many_sweeps=args.gibbs_ms * iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
