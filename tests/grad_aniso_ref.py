"""numpy restatement of the per-axis gradient sweep (nngp_bf_grad_aniso): tests/test_gpu_grad.py::ref_rows' scalar-loop
structure with one derivative block D_k per axis.  Shared by test_grad_aniso_host.py (which pins it) and
test_gpu_grad_aniso.py (which compares the GPU with it)."""
import numpy as np

from test_gpu_grad import chol_solve, rho_drho

KINDS = ("exponential", "matern32", "matern52", "gaussian", "spherical")


def ref_rows_aniso(coords, nbr, kind, theta, y, rows=None, dtype=np.float64):
    """Per-location (log F, r^2/F, G[dim + 2]) for theta = (sigma2, phi_1 .. phi_dim, tau2), fp64 (or its
    ``np.longdouble`` twin: the same code on extended-precision inputs).  With delta = phi * (x_a - x_b) and
    u = |delta|: C = sigma2 rho(u) + tau2 I and D_k = sigma2 rho'(u) delta_k^2 / (u phi_k), 0 where u = 0."""
    coords, y = coords.astype(dtype), y.astype(dtype)
    dim = coords.shape[1]
    s2, t2 = dtype(theta[0]), dtype(theta[-1])
    phi = np.array(theta[1:-1], dtype=dtype)
    assert phi.shape == (dim,)
    rows = range(coords.shape[0]) if rows is None else rows
    out = np.zeros((len(rows), 4 + dim), dtype=dtype)
    for t, i in enumerate(rows):
        nb = [j for j in nbr[i] if j >= 0]
        k = len(nb)
        idx = nb + [i]
        X = coords[idx] * phi
        delta2 = (X[:, None, :] - X[None, :, :]) ** 2
        u = np.sqrt(delta2.sum(-1))
        r_, dr_ = rho_drho(kind, u)
        C = s2 * r_ + t2 * np.eye(k + 1, dtype=dtype)
        safe = np.where(u > 0, u, dtype(1.0))
        w = np.where(u > 0, s2 * dr_ / safe, dtype(0.0))
        D = [w * delta2[:, :, a] / phi[a] for a in range(dim)]
        yy = y[idx]
        if k:
            sol = chol_solve(C[:k, :k], np.stack([C[:k, k], yy[:k]], 1))
            b, a = sol[:, 0], sol[:, 1]
        else:
            b = a = np.zeros(0, dtype=dtype)
        uu = np.append(-b, dtype(1.0))
        al = np.append(a, dtype(0.0))
        F = uu @ C @ uu
        r = yy[k] - b @ yy[:k]
        nb2, adb = b @ b, a @ b
        dF = [(F - t2 * (1 + nb2)) / s2] + [uu @ Dk @ uu for Dk in D] + [1 + nb2]
        dr = [-t2 * adb / s2] + [-(al @ Dk @ uu) for Dk in D] + [adb]
        out[t, 0], out[t, 1] = np.log(F), r * r / F
        for p in range(dim + 2):
            out[t, 2 + p] = -0.5 * ((dF[p] / F) * (1 - r * r / F) + 2 * r * dr[p] / F)
    return out


def field(n, dim=2, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (n, dim)), rng.standard_normal(n)


# the GPU parity test's inputs (test_gpu_grad_aniso.py) and the host test that conditions its tolerance
PARITY_PHI = (3.0, 9.0)
PARITY_SEED = 1


def parity_theta(kind, phi=PARITY_PHI):
    # the spherical kind's range is 1 / phi_k per axis: smaller decays keep most pairs inside u < 1
    if kind == "spherical":
        return (1.3, *(p / 4.0 for p in phi), 0.05)
    return (1.3, *phi, 0.05)
