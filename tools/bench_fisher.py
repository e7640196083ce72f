#!/usr/bin/env python3
"""Time the Fisher information sweep (nngp_bf_fisher) beside the gradient sweep (nngp_bf_grad) and the
phi-derivative sweep (nngp_bf_dphi) in one process: warm launches of each first, then event-bracketed rounds that
alternate the three.  Then fit(method="fisher") against fit(gradient=True) at a small n: sweeps (kernel launches of
the bf family, counted at the binding) and wall time, both from the same start.  Records the library's size.
Writes profiles/fisher/bench_fisher.json and prints it as one JSON line.

python tools/bench_fisher.py [--n 1000000] [--m 10 15 20 32] [--kind exponential] [--fit-n 2000]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pynngp_amd import _lib  # noqa: E402
from pynngp_amd import nngp as N  # noqa: E402

PARENT_LIB_BYTES = 54_634_344  # libnngp_hip.so before the bf_fisher units


def time_ms(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def sweeps(a, dev):
    rng = np.random.default_rng(0)
    coords = torch.from_numpy(rng.uniform(0.0, 1.0, (a.n, 2))).to(dev)
    y = torch.from_numpy(rng.standard_normal(a.n)).to(dev)
    lib = _lib.load()
    out = []
    for m in a.m:
        nbr = _lib.knn_prior(coords, m)
        order, nbs = _lib.row_order(coords, 0, a.n, nbr)
        del nbr
        wsg = _lib._workspace(lib.nngp_bf_grad_workspace_bytes(a.n, m), dev)
        wsd = _lib._workspace(lib.nngp_bf_dphi_workspace_bytes(a.n, m), dev)
        wsf = _lib._workspace(lib.nngp_bf_fisher_workspace_bytes(a.n, m), dev)
        B, dB = (torch.empty((a.n, m), dtype=torch.float64, device=dev) for _ in range(2))
        F, dF = (torch.empty(a.n, dtype=torch.float64, device=dev) for _ in range(2))

        def grad():
            return _lib.bf_grad(coords, nbs, 0, a.kind, *a.theta, y, order=order, workspace=wsg)

        def dphi():
            return _lib.bf_dphi(coords, nbs, 0, a.kind, *a.theta, order=order, B=B, F=F, dB=dB, dF=dF, workspace=wsd)

        def fisher():
            return _lib.bf_fisher(coords, nbs, 0, a.kind, *a.theta, y, order=order, workspace=wsf)

        fns = {"fisher": fisher, "grad": grad, "dphi": dphi}
        for fn in fns.values():
            time_ms(fn, a.warmup)
        t = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                t[k].append(time_ms(fn, a.launches))
        p, g, info, _, _ = fisher()
        pg, gg, _ = grad()
        med = {k: float(np.median(v)) for k, v in t.items()}
        out.append({"m": m, **{f"{k}_ms": med[k] for k in fns}, **{f"{k}_ms_min": min(t[k]) for k in fns},
                    "fisher_over_grad": med["fisher"] / med["grad"],
                    "fisher_over_grad_plus_dphi": med["fisher"] / (med["grad"] + med["dphi"]),
                    "info": info.cpu().numpy().tolist(),
                    "grad_rel_diff_vs_bf_grad": float(torch.max(torch.abs(g - gg) / (1 + torch.abs(gg))).item())})
        del nbs, order, B, dB, F, dF
    return out


def fits(a, dev):
    """fit(method="fisher") and fit(gradient=True) on one simulated field, from the same start."""
    rng = np.random.default_rng(11)
    coords = rng.uniform(0.0, 1.0, (a.fit_n, 2))
    gen = N.NNGP(coords, np.zeros(a.fit_n), None, "S=T", 10, N.Covariance("exponential", 1.0, 12.0, 0.1), device=dev)
    y = gen.simulate(1, seed=7, beta=0.5)[0]
    counts = {}
    originals = {k: getattr(_lib, k) for k in ("bf_sweep", "bf_grad", "bf_fisher")}

    def counted(name):
        def call(*args, **kw):
            counts[name] = counts.get(name, 0) + 1
            return originals[name](*args, **kw)
        return call

    out = {}
    try:
        for k in originals:
            setattr(_lib, k, counted(k))
        for label, kw in (("fisher", dict(method="fisher")), ("lbfgsb_gradient", dict(gradient=True))):
            best = None
            for rep in range(a.fit_reps):  # the first repetition warms every kernel the fit uses
                counts.clear()
                model = N.NNGP(coords, y, None, "S=T", 10, N.Covariance("exponential", 0.5, 5.0, 0.3), device=dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = model.fit(**kw)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                best = wall if best is None or rep == 1 else min(best, wall)
            out[label] = {"wall_s_min_after_warmup": best, "sweeps": dict(counts), "sweeps_total": sum(counts.values()),
                          "n_evals": res["n_evals"], "n_iter": res.get("n_iter"), "loglik": res["loglik"],
                          "theta": list(res["theta"]), "converged": res["converged"],
                          "se": None if "se" not in res else np.asarray(res["se"]).tolist()}
    finally:
        for k, fn in originals.items():
            setattr(_lib, k, fn)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, nargs="+", default=[10, 15, 20, 32])
    ap.add_argument("--kind", default="exponential")
    ap.add_argument("--theta", type=float, nargs=3, default=[1.0, 30.0, 0.1])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fit-n", type=int, default=2000)
    ap.add_argument("--fit-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fisher", "bench_fisher.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fisher needs a GPU")
    dev = torch.device("cuda", 0)
    size = os.path.getsize(_lib.LIB_PATH)
    doc = {"tool": "bench_fisher", "n": a.n, "kind": a.kind, "theta": a.theta, "launches": a.launches,
           "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "library_bytes": size, "library_bytes_parent": PARENT_LIB_BYTES, "library_bytes_added": size - PARENT_LIB_BYTES,
           "sweeps": sweeps(a, dev), "fit_n": a.fit_n, "fit": fits(a, dev)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
