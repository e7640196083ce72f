"""GPU: the latent calls at one right-hand side reproduce, bit for bit, what the separate single-RHS kernels of
commit dd168c1 computed.

tests/golden/latent_single_pin.npz (written by tests/golden/make_latent_pin.py on that commit) holds the inputs
and the outputs of ``precision_apply``, ``precision_sqrt_t_apply`` and ``latent_cg`` on the smallest shapes at
which a kernel can go wrong: n = 1; m = 32 with a ragged last tile; the 4- and 8-lane row groups; -1 slots in
the middle of a row; two reverse lists above the block-cooperative threshold in one tile; solves with
check_every 1 and 8, from a non-zero start, cut off by max_iter, and broken down by a NaN.  Each output must be
reproduced by the single wrapper, by the batched wrapper at nrhs = 1, and by column 1 of the batched wrapper at
nrhs = 3 (other columns random): the kernels are one template family, and a column's bits depend neither on the
instantiation that serves it nor on its neighbours.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _pin():
    return load_golden("latent_single_pin")


@functools.lru_cache(maxsize=None)
def _geometry(dev, g):
    from pynngp_amd import _lib

    pin = _pin()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    nbr, B = to(pin[f"{g}.nbr"]), to(pin[f"{g}.B"])
    off, rev_j, rev_k = _lib.reverse_neighbors(nbr)
    prep = _lib.gibbs_prepare(B, to(pin[f"{g}.F"]), off, rev_j, rev_k)
    return nbr, B, off, rev_j, rev_k, prep, float(pin["sigma2"])


def _dt(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _widen(v, dev, seed):
    """(n, 3) device columns with v in column 1 and random columns on other scales beside it."""
    if v is None:
        return None
    rng = np.random.default_rng(seed)
    cols = np.stack([1e3 * rng.standard_normal(v.shape[0]), v, 1e-3 * rng.standard_normal(v.shape[0])], axis=1)
    return _dt(cols, dev)


def _col(v, dev):
    return None if v is None else _dt(v[:, None], dev)


OP_CASES = [(str(g), tag) for g in _pin()["geom_names"] for tag in ("d0", "d1")]


@pytest.mark.parametrize("g,tag", OP_CASES)
def test_operators_reproduce_the_pinned_bits(dev, g, tag):
    from pynngp_amd import _lib

    pin, geom = _pin(), _geometry(dev, g)
    key = f"op.{g}.{tag}."
    x = pin[f"op.{g}.x"]
    z2, d = (pin[f"op.{g}.z2"], pin[f"op.{g}.d"]) if tag == "d1" else (None, None)
    d_d = _dt(d, dev)
    want = {"apply": pin[key + "apply"], "sqrt": pin[key + "sqrt"]}
    got = {"apply": _lib.precision_apply(*geom, _dt(x, dev), d=d_d),
           "sqrt": _lib.precision_sqrt_t_apply(*geom, _dt(x, dev), _dt(z2, dev), d=d_d)}
    got1 = {"apply": _lib.precision_apply_batch(*geom, _col(x, dev), d=d_d)[:, 0],
            "sqrt": _lib.precision_sqrt_t_apply_batch(*geom, _col(x, dev), _col(z2, dev), d=d_d)[:, 0]}
    got3 = {"apply": _lib.precision_apply_batch(*geom, _widen(x, dev, 1), d=d_d)[:, 1],
            "sqrt": _lib.precision_sqrt_t_apply_batch(*geom, _widen(x, dev, 1), _widen(z2, dev, 2), d=d_d)[:, 1]}
    for op in ("apply", "sqrt"):
        np.testing.assert_array_equal(got[op].cpu().numpy(), want[op], err_msg=f"{op} {g} {tag}: single call")
        np.testing.assert_array_equal(got1[op].cpu().numpy(), want[op], err_msg=f"{op} {g} {tag}: nrhs = 1")
        np.testing.assert_array_equal(got3[op].cpu().numpy(), want[op], err_msg=f"{op} {g} {tag}: column 1 of 3")


@pytest.mark.parametrize("name", [str(c) for c in _pin()["cg_names"]])
def test_cg_reproduces_the_pinned_bits(dev, name):
    pin = _pin()
    key = f"cg.{name}."
    g = str(pin[key + "geom"])
    geom = _geometry(dev, g)
    b = pin.get(key + "b", pin[f"rhs.{g}.b"])
    x0 = pin.get(key + "x0", np.zeros_like(b))
    kw = dict(d=_dt(pin[f"rhs.{g}.d"], dev), rtol=float(pin[key + "rtol"]), max_iter=int(pin[key + "max_iter"]))
    want_x, want_info = pin[key + "x"], pin[key + "info"]
    print(f"{name}: pinned info {want_info.tolist()}")
    for ce in pin[key + "check_every"].tolist():
        kw["check_every"] = ce
        _check_cg(dev, geom, b, x0, kw, want_x, want_info, f"{name}, check_every {ce}")


def _check_cg(dev, geom, b, x0, kw, want_x, want_info, name):
    from pynngp_amd import _lib

    x, info = _lib.latent_cg(*geom, _dt(b, dev), _dt(x0, dev), **kw)
    np.testing.assert_array_equal(np.array(info), want_info, err_msg=f"{name}: single call")
    np.testing.assert_array_equal(x.cpu().numpy(), want_x, err_msg=f"{name}: single call")

    x, info = _lib.latent_cg_batch(*geom, _col(b, dev), _col(x0, dev), **kw)
    np.testing.assert_array_equal(info[0], want_info, err_msg=f"{name}: nrhs = 1")
    np.testing.assert_array_equal(x[:, 0].cpu().numpy(), want_x, err_msg=f"{name}: nrhs = 1")

    x, info = _lib.latent_cg_batch(*geom, _widen(b, dev, 3), _widen(x0, dev, 4), **kw)
    np.testing.assert_array_equal(info[1], want_info, err_msg=f"{name}: column 1 of 3")
    np.testing.assert_array_equal(x[:, 1].cpu().numpy(), want_x, err_msg=f"{name}: column 1 of 3")


def test_the_pin_holds_the_cases_it_is_meant_to():
    """The fixture itself: the statuses that make the cut-off and breakdown cases what they are."""
    pin = _pin()
    assert pin["cg.max_iter3.info"].tolist()[:2] == [3.0, 0.0]
    assert pin["cg.nan_b.info"][1] == -1.0 and np.isnan(pin["cg.nan_b.b"]).sum() == 1
    assert np.any(pin["cg.x0.x0"] != 0.0) and pin["cg.x0.info"][1] == 1.0
    for g in ("f400_8", "twohub600_4"):
        assert pin[f"cg.{g}.info"][1] == 1.0 and pin[f"cg.{g}.check_every"].tolist() == [1, 8]
    deg = np.bincount(pin["twohub600_4.nbr"][pin["twohub600_4.nbr"] >= 0], minlength=600)
    assert deg[0] == deg[1] == 598
