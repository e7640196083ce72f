"""CPU: what the binomial latent posterior refuses before any device work -- the C-ABI argument checks of
nngp_binomial_newton_step / nngp_logistic_normal (a negative count lives in device memory, so the C ABI refuses it
through the host helper nngp_binomial_check_partials on the call's partials), the CPU-tensor refusals of the Python
wrappers and the torch operators, and the constructor's validation of successes and trials."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from pynngp_amd import _lib

    return _lib.load()


def _step(lib, n=10, ws_bytes=1 << 12, **null):
    P = lambda name: None if name in null else ctypes.c_void_p(256)  # noqa: E731  (never dereferenced: refused first)
    return lib.nngp_binomial_newton_step(n, P("trials"), P("successes"), P("offset"), P("w"), P("d"), P("rhs"), P("g"),
                                         P("partials"), P("workspace"), ws_bytes, None)


@pytest.mark.parametrize("name", ["trials", "successes", "offset", "w", "d", "rhs", "g", "partials", "workspace"])
def test_newton_step_refuses_null_pointers(lib, name):
    assert _step(lib, **{name: True}) == -1
    assert b"null pointer" in lib.nngp_last_error()


def test_newton_step_refuses_bad_n_and_small_workspace(lib):
    assert _step(lib, n=-1) == -1 and b"bad n=-1" in lib.nngp_last_error()
    assert _step(lib, n=2 ** 31 - 1) == -1 and b"bad n=" in lib.nngp_last_error()
    assert lib.nngp_binomial_newton_step_workspace_bytes(-1) == 0
    assert lib.nngp_binomial_newton_step_workspace_bytes(257) == 256  # two 32-B block records, 256-B granules
    assert lib.nngp_binomial_newton_step_workspace_bytes(65537) == 257 * 32 + (256 - 257 * 32 % 256)
    assert _step(lib, n=65537, ws_bytes=256) == -1 and b"workspace too small" in lib.nngp_last_error()


def test_negative_trials_and_nonfinite_eta_are_refused_from_the_partials(lib):
    from pynngp_amd import _lib

    a, b = ctypes.c_int64(7), ctypes.c_int64(7)
    chk = lambda p: lib.nngp_binomial_check_partials(  # noqa: E731
        ctypes.cast((ctypes.c_double * 4)(*p), ctypes.c_void_p), ctypes.cast(ctypes.byref(a), ctypes.c_void_p),
        ctypes.cast(ctypes.byref(b), ctypes.c_void_p))
    assert chk([-3.5, 0.2, 0.0, 0.0]) == 0 and (a.value, b.value) == (-1, -1)
    assert chk([-3.5, 0.2, 0.0, 12.0]) == -1 and b"negative trials at node 11" in lib.nngp_last_error()
    assert (a.value, b.value) == (-1, 11)
    assert chk([-3.5, 0.2, 5.0, 0.0]) == -1 and b"not finite at node 4" in lib.nngp_last_error()
    assert (a.value, b.value) == (4, -1)
    assert lib.nngp_binomial_check_partials(None, None, None) == -1 and b"non-null" in lib.nngp_last_error()
    assert _lib.binomial_check_partials([0.0, 0.0, 3.0, 9.0]) == (2, 8)


def test_logistic_normal_refuses_null_pointers_and_bad_n(lib):
    P = ctypes.c_void_p(256)
    for args in ((None, P, P), (P, None, P), (P, P, None)):
        assert lib.nngp_logistic_normal(4, *args, None) == -1 and b"null pointer" in lib.nngp_last_error()
    assert lib.nngp_logistic_normal(-2, P, P, P, None) == -1 and b"bad n=-2" in lib.nngp_last_error()


def test_wrappers_and_ops_refuse_cpu_tensors():
    from pynngp_amd import _lib, load_ops

    load_ops()
    t = torch.ones(5, dtype=torch.int32)
    v = torch.zeros(5, dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        _lib.binomial_newton_step(t, v, v, v)
    with pytest.raises(NotImplementedError):
        _lib.logistic_normal(v, v)
    with pytest.raises(NotImplementedError):
        torch.ops.nngp.binomial_newton_step(t, v, v, v)
    with pytest.raises(NotImplementedError):
        torch.ops.nngp.logistic_normal(v, v)
    for name in ("binomial_newton_step", "logistic_normal"):
        assert hasattr(torch.ops.nngp, name)


@pytest.mark.parametrize("succ,trials,msg", [
    ([0.5, 1, 0, 1], [1, 1, 1, 1], "successes must be integers"),
    ([2, 1, 0, 1], [1, 1, 1, 1], r"successes must lie in \[0, trials\]"),
    ([-1, 1, 0, 1], [1, 1, 1, 1], r"successes must lie in \[0, trials\]"),
    ([0, 1, 0, 1], [1, -1, 1, 1], "trials must lie in"),
    ([0, 1, 0, 1], [1, 1.5, 1, 1], "trials must be integers"),
    ([0, 1, 0, np.inf], [1, 1, 1, 1], "finite or NaN"),
    ([0, 1, 0], [1, 1, 1, 1], "one count per location"),
    ([np.nan] * 4, [1, 1, 1, 1], "no observed responses"),
    ([0, 1, 0, 1], [0, 0, 0, 0], "no observed responses"),
])
def test_constructor_refuses_bad_counts(succ, trials, msg):
    from pynngp_amd import BinomialLatentPosterior, Covariance

    coords = np.random.default_rng(0).uniform(size=(4, 2))
    with pytest.raises(ValueError, match=msg):
        BinomialLatentPosterior(coords, succ, trials, Covariance("exponential", 1.0, 5.0, 0.0), m=2)


def test_constructor_takes_trials_beyond_the_sampler_cap_and_refuses_a_callable_cov():
    from pynngp_amd import BinomialLatentPosterior
    from pynngp_amd.latent_binomial import _check_counts

    s, b, obs = _check_counts([5000, 0, np.nan], [10 ** 6, 3, 7], 3)  # BinomialSeqNNGP stops at 1024
    assert b.tolist() == [10 ** 6, 3, 7] and obs.tolist() == [True, True, False]
    with pytest.raises(TypeError, match="Covariance"):
        BinomialLatentPosterior(np.zeros((3, 2)), [1, 0, 1], [1, 1, 1], lambda a, b: a)
