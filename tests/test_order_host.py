"""CPU: the levelled max-min order as tests/order_ref.py restates it -- it is a permutation, separates and covers
at every level, stays within a factor 4 of the exact greedy max-min distances, handles lattices, duplicates and
degenerate sets -- plus the refusals of pynngp_amd.ordering, the unchanged ordering=None path of NNGP, and the
host arithmetic of the HIP unit (pynngp_amd/csrc/order_maxmin.h) under AddressSanitizer +
UndefinedBehaviorSanitizer in a stand-alone program (tests/host/order_check.cpp; never loaded into Python)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import order_ref as R
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", ["uniform1d", "uniform2d", "uniform3d"])
def test_uniform_properties_and_greedy_bound(name):
    x = R.case(name)
    perm, level = R.reference(name)
    R.check_properties(x, perm, level)
    lo, med = R.greedy_ratio(x, perm, level)
    print(f"{name}: min s_k/g_k = {lo:.3f}, median {med:.3f}")
    assert lo >= 0.25  # the proven bound (Gonzalez's 2-approximation and the covering radius 2 r_l)
    assert med >= 0.5


def test_lattice_exact_ties():
    """A 32 x 32 integer lattice: many pairs are at exactly r of a level (dist2 == r2 counts as separated)."""
    x = R.case("lattice32")
    perm, level = R.reference("lattice32")
    R.check_properties(x, perm, level)
    lo, _ = R.greedy_ratio(x, perm, level)
    print(f"lattice32: min s_k/g_k = {lo:.3f}")
    assert lo >= 0.25


def test_duplicates_go_to_the_tail():
    x = R.case("duplicates")
    perm, level = R.reference("duplicates")
    R.check_properties(x, perm, level)
    tail = perm[level == R.TAIL]
    assert tail.size == 100
    body = perm[level < R.TAIL]
    # one of each coincident pair is in the body, the other in the tail
    body_pts = {tuple(p) for p in x[body]}
    assert len(body_pts) == 300 and all(tuple(p) in body_pts for p in x[tail])
    assert np.array_equal(tail, tail[np.argsort(R.keys(len(x))[tail])])  # the tail is in key order


def test_degenerate_sets():
    perm, level = R.reference("one")
    assert perm.tolist() == [0] and level.tolist() == [0]
    perm, level = R.reference("two")  # both points are equally far from the centre: p1 is row 0
    assert perm.tolist() == [0, 1] and level.tolist() == [0, 1]
    x = R.case("coincident")
    perm, level = R.reference("coincident")
    key = R.keys(len(x))
    rest = np.arange(1, len(x))
    assert perm[0] == 0 and level[0] == 0 and np.all(level[1:] == R.TAIL)  # R = 0: everything else is the tail
    assert np.array_equal(perm[1:], rest[np.argsort(key[rest])])


def test_levels_are_key_sorted_and_seed_changes_the_order():
    x = R.case("uniform2d")
    perm, level = R.reference("uniform2d")
    key = R.keys(len(x))
    for l in np.unique(level):
        k = key[perm[level == l]]
        assert np.all(k[1:] > k[:-1])
    perm7, level7 = R.reference("uniform2d", seed=7)
    assert not np.array_equal(perm7, perm)
    R.check_properties(x, perm7, level7)
    lo, _ = R.greedy_ratio(x, perm7, level7)
    assert lo >= 0.25
    assert np.array_equal(np.sort(R.order_random(1500, 3)), np.arange(1500))
    assert not np.array_equal(R.order_random(1500, 3), R.order_random(1500, 4))


def test_key_is_the_murmur3_finaliser():
    # mix32 of 0, 1 and 0xdeadbeef from the murmur3 reference implementation's fmix32
    assert [int(v) for v in R.mix32(np.array([0, 1, 0xDEADBEEF]))] == [0, 0x514E28B7, 0x0DE5C6A9]
    k = R.keys(4, seed=2)
    assert [int(v) & 0xFFFFFFFF for v in k] == [0, 1, 2, 3]
    assert int(k[1]) >> 32 == int(R.mix32(np.array([(1 + 2 * 0x9E3779B9) & 0xFFFFFFFF]))[0])


def test_api_refusals():
    import pynngp_amd
    from pynngp_amd import _lib, ordering

    ok = torch.rand((40, 2), dtype=torch.float64)
    with pytest.raises(_lib.NNGPExtensionError, match="no CPU fallback"):
        pynngp_amd.order_maxmin(ok)
    with pytest.raises(_lib.NNGPExtensionError, match="no CPU fallback"):
        pynngp_amd.order_coordinate(ok)
    with pytest.raises(_lib.NNGPExtensionError, match="no CPU fallback"):
        pynngp_amd.order_middleout(ok)
    with pytest.raises(_lib.NNGPExtensionError, match="no CPU fallback"):
        pynngp_amd.order_random(40, 0, device="cpu")
    with pytest.raises(ValueError, match="dim"):
        pynngp_amd.order_maxmin(torch.rand((40, 4), dtype=torch.float64))
    with pytest.raises(ValueError):
        pynngp_amd.order_maxmin(torch.rand((40, 2), dtype=torch.float32))
    for bad in (float("nan"), float("inf")):
        c = ok.clone()
        c[3, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            pynngp_amd.order_maxmin(c)
    with pytest.raises(ValueError, match="uint32"):
        pynngp_amd.order_random(40, -1, device="cuda")
    with pytest.raises(ValueError, match="length 40"):
        ordering.check_permutation(np.arange(39), 40)
    with pytest.raises(ValueError, match="permutation of range"):
        ordering.check_permutation(np.zeros(40, dtype=np.int64), 40)
    with pytest.raises(ValueError, match="integers"):
        ordering.check_permutation(np.arange(40.0), 40)
    with pytest.raises(ValueError, match="unknown ordering"):
        ordering.resolve("hilbert", ok)
    assert np.array_equal(ordering.check_permutation(torch.arange(40).flip(0), 40), np.arange(40)[::-1])


def test_c_abi_refusals():
    import ctypes

    from pynngp_amd import _lib

    lib = _lib.load()
    P = ctypes.c_void_p
    assert lib.nngp_order_maxmin_workspace_bytes(0, 2) == 0
    assert lib.nngp_order_maxmin_workspace_bytes(100, 4) == 0
    assert lib.nngp_order_maxmin_workspace_bytes(100, 0) == 0
    need = lib.nngp_order_maxmin_workspace_bytes(100, 2)
    assert need > 0 and need % 256 == 0
    good = dict(coords=P(256), n=100, dim=2, seed=0, perm=P(256), level=P(256), ws=P(256), ws_bytes=need)
    for kw in (dict(coords=None), dict(perm=None), dict(level=None), dict(ws=None), dict(dim=0), dict(dim=4),
               dict(n=0), dict(n=-5), dict(n=2 ** 31), dict(ws_bytes=need - 1), dict(ws=P(257))):
        a = dict(good, **kw)
        rc = lib.nngp_order_maxmin(a["coords"], a["n"], a["dim"], a["seed"], a["perm"], a["level"], a["ws"],
                                   a["ws_bytes"], None)
        assert rc == -1, kw  # NNGP_EINVAL, before any device call


def test_ops_schema_and_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from pynngp_amd import load_ops

    load_ops()
    assert "order_maxmin(Tensor coords, int seed) -> (Tensor, Tensor)" in str(
        torch.ops.nngp.order_maxmin.default._schema)
    with pytest.raises(NotImplementedError):
        torch.ops.nngp.order_maxmin(torch.rand((50, 2), dtype=torch.float64), 0)
    with FakeTensorMode():
        perm, level = torch.ops.nngp.order_maxmin(torch.empty((64, 3), dtype=torch.float64), 0)
    assert tuple(perm.shape) == (64,) and perm.dtype == torch.int64
    assert tuple(level.shape) == (64,) and level.dtype == torch.int32


def _bare_model(n=12, dim=2, m=3):
    """An NNGP with its attributes set and nothing built on a GPU (as tests/test_grad_aniso_host.py does)."""
    from pynngp_amd import nngp as N

    model = object.__new__(N.NNGP)
    model.cov, model.m, model.refType, model.device = None, m, "S=T", torch.device("cpu")
    model.t = model.s = np.arange(n * dim, dtype=np.float64).reshape(n, dim)
    model.y, model.eps = np.arange(n, dtype=np.float64), None
    return model


def test_ordering_none_takes_the_old_path(monkeypatch):
    """Without an ordering the constructor does not touch pynngp_amd.ordering, t / y are the caller's own objects,
    perm is None and the two converters are the identity."""
    import inspect

    from pynngp_amd import nngp as N
    from pynngp_amd import ordering

    assert inspect.signature(N.NNGP.__init__).parameters["ordering"].default is None

    def boom(*a, **k):
        raise AssertionError("ordering=None must not compute an ordering")

    monkeypatch.setattr(ordering, "resolve", boom)
    monkeypatch.setattr(N.NNGP, "_order_inputs", boom)
    monkeypatch.setattr(N.NNGP, "_order_reference", boom)
    model = _bare_model()
    t, y = model.t, model.y
    model.perm, model._ordering = None, None
    model._init_s()
    assert model.t is t and model.s is t and model.y is y
    a = np.arange(12.0)
    assert model.to_model_order(a) is a and model.to_input_order(a) is a
    # and the full constructor reaches the device check exactly as before when there is no GPU
    if not torch.cuda.is_available():
        with pytest.raises(N._lib.NNGPExtensionError, match="needs a ROCm GPU"):
            N.NNGP(t, y, None, "S=T", 3, None)
        with pytest.raises(N._lib.NNGPExtensionError, match="needs a ROCm GPU"):
            N.NNGP(t, y, None, "S=T", 3, None, ordering="maxmin")


def test_model_order_converters_roundtrip():
    model = _bare_model()
    perm = np.random.default_rng(0).permutation(12)
    model.perm = torch.as_tensor(perm)
    a = np.random.default_rng(1).normal(size=(12, 3))
    assert np.array_equal(model.to_model_order(a), a[perm])
    assert np.array_equal(model.to_input_order(model.to_model_order(a)), a)
    ta = torch.as_tensor(a)
    assert torch.equal(model.to_input_order(model.to_model_order(ta)), ta)


def test_reference_set_maxmin_branch_is_new_and_others_unchanged():
    from pynngp_amd.nngp import reference_set

    t = np.random.default_rng(0).uniform(size=(30, 2))
    assert reference_set(t, "S=T") is t
    np.random.seed(3)
    s = reference_set(t, ("subset", 7))
    np.random.seed(3)
    assert np.array_equal(s, t[np.random.choice(30, size=7)])
    with pytest.raises(ValueError, match="maxmin"):
        reference_set(t, ("grid", 3))
    if not torch.cuda.is_available():
        with pytest.raises(Exception, match="ROCm GPU"):
            reference_set(t, ("maxmin", 5))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_host_arithmetic_under_sanitizers(tmp_path):
    """order_maxmin.h's key, level radii and table sizing in a stand-alone program built with
    -fsanitize=address,undefined; it prints the keys and radii this test compares with the restatement's."""
    exe = tmp_path / "order_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "pynngp_amd", "csrc"), os.path.join(HERE, "host", "order_check.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out[0] == "ok"
    got_keys = [int(v, 16) for v in out[1:9]]
    assert got_keys == [int(v) for v in R.keys(4, 0)] + [int(v) for v in R.keys(4, 5)]
    # level 7 of R = 3.7 in 2-D: r2 and h as floats' hex
    r = np.ldexp(3.7, -7)
    assert [float.fromhex(out[9]), float.fromhex(out[10])] == [r * r, r * 0.7]
