#!/usr/bin/env python3
"""Times the levelled max-min ordering (nngp_order_maxmin) and what the order of the points does to the rest of a
model build, and writes profiles/order/bench_order.json.

Per case (N = 1e6 and 1e7 in 2-D, N = 1e6 in 3-D, uniform points):
* order_maxmin: ms per call, its launches, count reads and rounds / accept-retire iterations per level, beside
  nngp_knn_prior on the same points (the yardstick: the other once-per-data-set step of a build);
* under three orders of the same points -- as drawn, max-min, sorted by x -- the neighbour build (knn_prior) and
  the forward sweep (bf_sweep at m, exponential);
* with --factor (N = 1e6, 2-D only by default): NNGPFactor's depth / depth_t and one forward solve per order.
And once, at n = 900 (the set-up of tests/test_gpu_order.py): KL(exact || NNGP) under the three orders.

Timing: every shape warmed by untimed calls, each sample bracketed by events on the stream, medians over --repeats
rounds in which the variants alternate, all in one process.

    python tools/bench_order.py [--cases 2:1000000 2:10000000 3:1000000] [--m 15] [--out profiles/order/bench_order.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(fns, repeats, warmup=2):
    """Median ms of every named callable; the callables take turns inside each round."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(sample(fn))
    return {k: float(np.median(v)) for k, v in out.items()}


def measure(dim, n, args, dev):
    from pynngp_amd import _lib, order_coordinate

    rng = np.random.default_rng(dim * 1000 + 1)
    c = torch.from_numpy(rng.uniform(0.0, 1.0, (n, dim))).to(dev)
    v = torch.from_numpy(rng.standard_normal(n)).to(dev)
    perm, level, stats = _lib.order_maxmin(c, 0, want_stats=True)
    rec = {"dim": dim, "n": n, "m": args.m, "order_maxmin_stats": stats,
           "levels_used": int(level.max().item()), "workspace_bytes": int(
               _lib.load().nngp_order_maxmin_workspace_bytes(n, dim))}
    rec.update({f"{k}_ms": t for k, t in alternating(
        {"order_maxmin": lambda: _lib.order_maxmin(c, 0), "knn_prior_as_drawn": lambda: _lib.knn_prior(c, args.m)},
        args.repeats).items()})
    rec["order_maxmin_over_knn_prior"] = rec["order_maxmin_ms"] / rec["knn_prior_as_drawn_ms"]
    orders = {"as_drawn": c, "maxmin": c[perm].contiguous(), "sorted_x": c[order_coordinate(c, 0)].contiguous()}
    nbrs = {k: _lib.knn_prior(p, args.m) for k, p in orders.items()}
    theta = (1.0, args.phi, 0.05)
    rec["knn_prior_ms"] = alternating({k: (lambda p=p: _lib.knn_prior(p, args.m)) for k, p in orders.items()},
                                      args.repeats)
    rec["bf_sweep_ms"] = alternating(
        {k: (lambda p=p, k=k: _lib.bf_sweep(p, nbrs[k], 0, "exponential", *theta, values=v, want_bf=False))
         for k, p in orders.items()}, args.repeats)
    print({k: rec[k] for k in rec if k != "order_maxmin_stats"}, flush=True)
    print(stats, flush=True)
    if args.factor and (dim, n) in args.factor_cases:
        from pynngp_amd import Covariance, NNGPFactor

        fac = {}
        b = torch.from_numpy(rng.standard_normal((n, 1))).to(dev)
        for k, p in orders.items():
            f = NNGPFactor(p, Covariance("exponential", 1.0, args.phi), m=args.m, device=dev, nbr=nbrs[k])
            fac[k] = {"depth": int(f.depth), "depth_t": int(f.depth_t), "launches": f.n_launches,
                      "forward_solve_ms": alternating({"s": lambda f=f: f.solve(b)}, max(3, args.repeats // 2), 1)["s"]}
            print("factor", k, fac[k], flush=True)
            del f
        rec["factor"] = fac
    return rec


def kl_three_orders(dev):
    """KL(exact || NNGP) at n = 900 uniform 2-D, exponential (1, 6, 0.05), m = 10, B and F from the GPU."""
    from pynngp_amd import NNGP, Covariance

    coords = np.random.default_rng(31).uniform(size=(900, 2))
    theta = (1.0, 6.0, 0.05)
    out = {}
    for name, pts, ordering in (("sorted_x", coords[np.argsort(coords[:, 0], kind="stable")], None),
                                ("as_drawn", coords, None), ("maxmin", coords, "maxmin")):
        md = NNGP(pts, np.zeros(900), None, "S=T", 10, Covariance("exponential", *theta), device=dev,
                  ordering=ordering)
        x, nbr, B, F = np.asarray(md.t), md.nbr.cpu().numpy(), md.B.cpu().numpy(), md.F.cpu().numpy()
        n = len(x)
        d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
        Sigma = theta[0] * np.exp(-theta[1] * d) + theta[2] * np.eye(n)
        L = np.eye(n)
        for k in range(nbr.shape[1]):
            ok = nbr[:, k] >= 0
            L[np.flatnonzero(ok), nbr[ok, k]] -= B[ok, k]
        Q = L.T @ (L / F[:, None])
        out[name] = float(0.5 * (np.trace(Q @ Sigma) - n - (np.linalg.slogdet(Sigma)[1] - np.log(F).sum())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["2:1000000", "2:10000000", "3:1000000"], help="dim:n")
    ap.add_argument("--m", type=int, default=15)
    ap.add_argument("--phi", type=float, default=30.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--factor", action="store_true", help="also the factor schedule and one solve per order")
    ap.add_argument("--factor-cases", nargs="+", default=["2:1000000"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order", "bench_order.json"))
    args = ap.parse_args()
    args.factor_cases = [tuple(int(v) for v in s.split(":")) for s in args.factor_cases]
    if not torch.cuda.is_available():
        raise SystemExit("bench_order.py needs a ROCm GPU: timings come from the device or not at all")
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "kind": "exponential", "phi": args.phi,
           "yardstick": "knn_prior_as_drawn_ms: the neighbour build of the same points, timed in alternation",
           "kl_exact_to_nngp_n900_m10": kl_three_orders(dev), "runs": []}
    print(out["kl_exact_to_nngp_n900_m10"], flush=True)

    def dump():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    for case in args.cases:
        dim, n = (int(v) for v in case.split(":"))
        out["runs"].append(measure(dim, n, args, dev))
        dump()  # after every case: a run cut short still leaves what it measured
    if not args.factor:
        out["factor"] = "not run (--factor)"
    dump()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
