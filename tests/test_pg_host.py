"""CPU: the Polya-Gamma sampler core (pynngp_amd/csrc/polya_gamma.h) compiled on the host.

tests/host/pg_check.cpp includes the header the GPU kernels include and draws N = 2^18 values per
(b, c) cell, b in {1, 2, 7, 64}, c in {0, 0.1, 1, 2.5, 10, 50, 1000}, with a fixed seed.  The bounds are the
sampling error of a correct sampler at 5 sigma against the closed forms of PG(b, c) (tests/pg_moments.py): with
~100 checks the false-failure chance of a fresh seed is below 1e-4, and the seed is fixed.
"""
import os
import subprocess

import pytest

import pg_moments as M

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "pg_check.cpp")


def _run(exe, *args):
    out = subprocess.run([exe, *args], check=True, capture_output=True, text=True).stdout.split()
    return {k: float(v) for k, v in zip(out[::2], out[1::2])}


@pytest.fixture(scope="module")
def pg(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pg") / "pg_check")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", SRC, "-o", exe, "-lm"], check=True)
    return _run(exe)


CELLS = [(b, c) for b in M.BS for c in M.CS]


@pytest.mark.parametrize("k", range(len(CELLS)))
def test_cell_moments(pg, k):
    b, c = CELLS[k]
    assert (pg[f"cell{k}_b"], pg[f"cell{k}_c"]) == (b, c) and pg["N"] == 2 ** M.LOG2_N and pg["cells"] == len(CELLS)
    assert pg[f"cell{k}_ok"] == 1 and pg[f"cell{k}_min"] > 0, "every draw finite and positive"
    assert pg[f"cell{k}_bad"] == 0, "no loop cap hit"
    M.check_cell(b, c, int(pg["N"]), pg[f"cell{k}_mean"], pg[f"cell{k}_var"], pg[f"cell{k}_m4"], pg[f"cell{k}_lap"])


def test_no_cap_hit_and_few_rounds(pg):
    """No cell hit a cap; the proposal loop (acceptance above 0.999) needed a handful of rounds, far from 256."""
    assert pg["cap_hits"] == 0
    print("largest proposal / truncated-IG / series rounds:", pg["max_prop"], pg["max_ig"], pg["max_series"])
    assert 1 <= pg["max_prop"] <= 8 and 1 <= pg["max_ig"] <= 64 and 1 <= pg["max_series"] <= 8


def test_edge_cases(pg):
    assert pg["b0_zero"] == 1 and pg["b0_blocks"] == 0 and pg["b0_bad"] == 0  # b = 0: exactly 0.0, nothing drawn
    assert pg["sign_symmetric"] == 1  # c and -c: identical bits
    assert pg["repeatable"] == 1 and pg["seed_changes"] == 1 and pg["iteration_changes"] == 1
    assert pg["location_changes"] == 1
    # NaN / inf c and a b outside [0, 1024]: NaN, flagged, before any loop (no round, no Philox block)
    assert pg["nonfinite_flagged"] == 1 and pg["nonfinite_blocks"] == 0 and pg["nonfinite_rounds"] == 0
    assert pg["bmax_ok"] == 1
    assert pg["sweep_c_ok"] == 1 and pg["sweep_c_bad"] == 0  # finite and positive for |c| <= 1000


def test_sanitized_build_runs_clean(tmp_path):
    """The same program under AddressSanitizer and UBSan, stand-alone (a host program with its own main; a
    smaller N: the sanitizers check every path the full run takes, the moments are the full run's business)."""
    exe = str(tmp_path / "pg_check_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-std=c++17", "-pthread", SRC, "-o", exe, "-lm"], check=True)
    r = _run(exe, "12")
    assert r["cap_hits"] == 0 and r["sign_symmetric"] == 1 and r["nonfinite_flagged"] == 1 and r["sweep_c_ok"] == 1
