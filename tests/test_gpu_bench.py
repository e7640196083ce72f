"""bench.py's JSON contract on the GPU: one line on stdout with the driver's keys, `roofline`
and `cpu_baseline`, for the headline preset (reduced N), config 2 and config 5 (the Gibbs preset,
reduced N) -- the runs the round-end driver and DESIGN.md quote.  `cpu_baseline` and config 5's
separately timed sweeps come with `--full`; a plain run leaves them out, and `--dump-outputs`
writes the last timed step's arrays, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline")


def _run(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra], capture_output=True, text=True,
                       timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]  # the JSON line is the only stdout output
    return json.loads(lines[0])


def _check(d, steps, warmup):
    for k in KEYS:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and "workload" in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert 0 < rf["frac"] < 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("port", "reference") and cb["sample"]


def test_bench_headline_contract(dev):
    d = _run("--full", "--steps", "20", "--warmup", "5", "--n", "200000", "--cpu-seconds", "0.3")
    _check(d, 20, 5)
    assert d["unit"] == "locations/s" and d["config"]["m"] == 15 and d["config"]["kind"] == "exponential"
    assert d["bad_rows"] == [-1, -1] and d["cpu_baseline"]["parity_max_rel_dF"] < 1e-10
    # the live kernel time at the driver's --steps 20: at least 5 event-bracketed samples, and the
    # per-launch loop time beside it
    rf = d["roofline"]
    assert rf["kernel_ms_samples"] >= 5 and rf["kernel_ms"] > 0 and rf["kernel_ms_loop_samples"] == 20
    assert rf["kernel_ms_loop"] > 0


def test_bench_config2_contract(dev):
    d = _run("--full", "--config", "2", "--steps", "20", "--warmup", "5", "--cpu-seconds", "0.3")
    _check(d, 20, 5)
    assert d["config"]["n_per_gpu"] == 100_000 and d["config"]["kind"] == "matern32"


def test_bench_config5_contract(dev):
    d = _run("--full", "--config", "5", "--steps", "5", "--warmup", "2", "--n", "20000", "--cpu-seconds", "0.3")
    _check(d, 5, 2)
    assert d["unit"] == "chain-iterations/s" and d["config"]["chains"] == 1
    b = d["breakdown"]
    assert b["n_colors"] > 0 and b["bf_sweep_ms"] > 0 and b["w_sweep_ms"] > 0  # (no timing bounds: a tiny N)


def test_bench_config5_two_chains_per_gpu(dev):
    d = _run("--full", "--config", "5", "--steps", "5", "--warmup", "2", "--n", "20000", "--cpu-seconds", "0",
             "--chains-per-gpu", "2")
    assert d["steps"] == 5 and d["value"] > 0 and d["config"]["chains"] == 2 and d["config"]["chains_per_gpu"] == 2


@pytest.mark.parametrize("mode", ["batched-streams", "batched", "batched-percopy", "streams"])
def test_bench_config5_chain_modes(dev, mode):
    d = _run("--full", "--config", "5", "--steps", "4", "--warmup", "2", "--n", "20000", "--cpu-seconds", "0",
             "--chains-per-gpu", "4", "--chain-mode", mode)
    assert d["steps"] == 4 and d["value"] > 0 and d["config"]["chains_per_gpu"] == 4
    assert d["config"]["chain_mode"] == mode


def _load(path):
    a = np.load(path, allow_pickle=False)
    assert a.dtype == np.float64, (path, a.dtype)
    return a


def test_bench_plain_run_dumps_last_step(dev, tmp_path):
    """A plain run: no CPU baselines, --steps timed steps, and --dump-outputs writes the last
    sweep's B, F, partials and log-likelihood -- bit-identical from one run to the next."""
    n = 50_001
    runs = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        d = _run("--steps", "7", "--warmup", "3", "--n", str(n), "--dump-outputs", str(out))
        for key in KEYS:
            assert key in d, key
        assert d["steps"] == 7 and d["warmup"] == 3 and d["ms_per_step"] > 0 and d["bad_rows"] == [-1, -1]
        assert d["roofline"]["kernel_ms_loop_samples"] == 7
        assert "cpu_baseline" not in d and "neighbor_build_cpu" not in d
        assert sorted(os.listdir(out)) == ["B.npy", "F.npy", "loglik.npy", "partials.npy"]
        a = {f[:-4]: _load(out / f) for f in os.listdir(out)}
        assert a["B"].shape == (n, 15) and a["F"].shape == (n,) and a["partials"].shape == (4,)
        assert np.isfinite(a["B"]).all() and (a["F"] > 0).all()
        assert float(a["loglik"]) == d["loglik"]
        assert d["loglik"] == -0.5 * (n * np.log(2 * np.pi) + a["partials"][0] + a["partials"][1])
        runs.append(a)
    for name in runs[0]:
        assert np.array_equal(runs[0][name], runs[1][name]), name


def test_bench_config5_plain_run_dumps_chain_state(dev, tmp_path):
    d = _run("--config", "5", "--steps", "5", "--warmup", "2", "--n", "20000", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 5 and d["ms_per_step"] > 0 and d["unit"] == "chain-iterations/s"
    assert d["roofline"] is None and "cpu_baseline" not in d and "bf_sweep_ms" not in d["breakdown"]
    assert sorted(os.listdir(tmp_path)) == ["beta.npy", "theta.npy", "w.npy"]
    w, beta, theta = (_load(tmp_path / f) for f in ("w.npy", "beta.npy", "theta.npy"))
    assert w.shape == (20000,) and np.isfinite(w).all() and w.std() > 0
    s = d["state"]
    assert list(beta) == s["beta"] and list(theta) == [s["sigma2"], s["phi"], s["tau2"]]
