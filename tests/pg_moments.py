"""Closed forms of PG(b, c) (Polson, Scott and Windle 2013) and the 5-sigma moment checks the CPU and GPU
Polya-Gamma tests share (tests/test_pg_host.py, tests/test_gpu_pg.py)."""
import math

BS = (1, 2, 7, 64)
CS = (0.0, 0.1, 1.0, 2.5, 10.0, 50.0, 1000.0)
LOG2_N = 18


def _logcosh(x):
    x = abs(x)
    return x + math.log1p(math.exp(-2.0 * x)) - math.log(2.0)


def pg_mean(b, c):
    return b / 4.0 if c == 0 else b / (2.0 * c) * math.tanh(0.5 * c)


def pg_var(b, c):
    """b (sinh c - c) sech^2(c/2) / (4 c^3), with sinh c sech^2(c/2) = 2 tanh(c/2) (no overflow at large c)"""
    if c == 0:
        return b / 24.0
    t = math.tanh(0.5 * c)
    return b * (2.0 * t - c * (1.0 - t * t)) / (4.0 * c ** 3)


def pg_laplace(b, c, t):
    """E exp(-t omega) = [cosh(c/2) / cosh(sqrt((c^2/2 + t)/2))]^b"""
    return math.exp(b * (_logcosh(0.5 * c) - _logcosh(math.sqrt(0.5 * (0.5 * c * c + t)))))


def check_cell(b, c, n, mean, var, m4, lap):
    """The issue's bounds: sample mean, E exp(-omega) and the sample variance within 5 standard errors
    (the variance's from the sample's own fourth central moment m4)."""
    ev, vv = pg_mean(b, c), pg_var(b, c)
    assert abs(mean - ev) <= 5.0 * math.sqrt(vv / n), ("mean", b, c, mean, ev, math.sqrt(vv / n))
    l1, l2 = pg_laplace(b, c, 1.0), pg_laplace(b, c, 2.0)
    se_l = math.sqrt(max(l2 - l1 * l1, 0.0) / n)
    assert abs(lap - l1) <= 5.0 * se_l, ("laplace", b, c, lap, l1, se_l)
    se_v = math.sqrt(max(m4 - var * var, 0.0) / n)
    assert abs(var - vv) <= 5.0 * se_v, ("variance", b, c, var, vv, se_v)
