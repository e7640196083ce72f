"""Numpy restatement of the Fisher information sweep (nngp_bf_fisher), shared by test_fisher_host.py and
test_gpu_fisher.py.

Two forms of a location's expected information in theta = (sigma2, phi, tau2), both batched over the locations
and written with a column-loop Cholesky and explicit substitutions (no LAPACK), so the same code runs in
``np.longdouble``:

* ``rows_bf``: the sweep's own quantities.  With C the joint block (neighbours, then the location; nugget on the
  whole diagonal), C_N = L L^T, b = C_N^-1 c, u = [-b; 1], F = u^T C u, D_ab = sigma2 d_ab rho'(phi d_ab),
  w = L^-1 (D u)[:k], t = L^-1 b, z = L^-1 y_N, r = y_i - b^T y_N:
      dF = ((F - tau2 (1 + |b|^2)) / sigma2, u^T D u, 1 + |b|^2),   W = ((tau2 / sigma2) t, w, -t)
      I[j, k] = 1/2 dF_j dF_k / F^2 + W_j . W_k / F
      G[j]    = -1/2 (dF_j / F) (1 - r^2 / F) + r (W_j . z) / F
* ``rows_trace``: 1/2 tr(A^-1 dA_j A^-1 dA_k) - 1/2 tr(N^-1 dN_j N^-1 dN_k), A the joint block and N its
  neighbour block (Guinness 2021).

Slots without a point (-1) are decoupled: their rows and columns of C are those of the identity and their
derivative entries are 0, so they add exactly 0 to every quantity, as in the kernel.
"""
import numpy as np

KINDS = ("exponential", "matern32", "matern52", "gaussian", "spherical")
THETA = (1.3, 6.0, 0.05)  # test_gpu_grad.py's
TRIU = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
HAVE_EXTENDED = np.finfo(np.longdouble).eps < 1e-18


def theta_of(kind):
    return (1.3, 1.7, 0.05) if kind == "spherical" else THETA


def field(n, dim=2, seed=0):
    """test_gpu_grad.py's field: uniform coordinates, then standard normal values."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (n, dim)), rng.standard_normal(n)


def knn_prior(coords, m):
    """Each point's min(m, i) nearest earlier points (squared distance, ties by index), -1 beyond."""
    n = len(coords)
    out = -np.ones((n, m), np.int32)
    for i in range(1, n):
        d = ((coords[:i] - coords[i]) ** 2).sum(1)
        o = np.argsort(d, kind="stable")[:m]
        out[i, :len(o)] = o
    return out


def full_sets(n):
    """m = n - 1: every earlier point, so the row sums are the dense GP's."""
    return np.array([[j if j < i else -1 for j in range(n - 1)] for i in range(n)], np.int32)


def rho_drho(kind, u):
    e = np.exp(-u)
    if kind == "exponential":
        return e, -e
    if kind == "matern32":
        return (1 + u) * e, -u * e
    if kind == "matern52":
        return (1 + u + u * u / 3) * e, -(u / 3) * (1 + u) * e
    if kind == "gaussian":
        g = np.exp(-u * u)
        return g, -2 * u * g
    inside = u < 1
    return np.where(inside, 1 - 1.5 * u + 0.5 * u**3, 0.0), np.where(inside, -1.5 + 1.5 * u * u, 0.0)


def chol(A):
    """Lower Cholesky factors of a batch (..., k, k), one column at a time."""
    k = A.shape[-1]
    L = np.zeros_like(A)
    for j in range(k):
        L[..., j, j] = np.sqrt(A[..., j, j] - (L[..., j, :j] ** 2).sum(-1))
        L[..., j + 1:, j] = (A[..., j + 1:, j] - (L[..., j + 1:, :j] * L[..., j:j + 1, :j]).sum(-1)) / L[..., j:j + 1, j]
    return L


def fwd(L, x):
    """L^-1 x for x (..., k, r)."""
    x = x.copy()
    for i in range(L.shape[-1]):
        x[..., i, :] = (x[..., i, :] - (L[..., i, :i, None] * x[..., :i, :]).sum(-2)) / L[..., i, i, None]
    return x


def bwd(L, x):
    """L^-T x for x (..., k, r)."""
    x = x.copy()
    for i in range(L.shape[-1] - 1, -1, -1):
        x[..., i, :] = (x[..., i, :] - (L[..., i + 1:, i, None] * x[..., i + 1:, :]).sum(-2)) / L[..., i, i, None]
    return x


def inv(A):
    L = chol(A)
    eye = np.broadcast_to(np.eye(A.shape[-1], dtype=A.dtype), A.shape)
    return bwd(L, fwd(L, eye))


def blocks(coords, nbr, kind, theta, dtype, rows=None):
    """Joint blocks of the rows: C (n, k+1, k+1) and its derivatives [dC/dsigma2, dC/dphi, dC/dtau2], with the
    slots without a point decoupled, and the (n, k+1) index and validity arrays."""
    coords = coords.astype(dtype)
    s2, phi, t2 = (dtype(x) for x in theta)
    rows = np.arange(len(nbr)) if rows is None else np.asarray(rows)
    idx = np.concatenate([nbr[rows], rows[:, None].astype(nbr.dtype)], 1)
    ok = idx >= 0
    X = coords[np.where(ok, idx, 0)]
    d = np.sqrt(((X[:, :, None, :] - X[:, None, :, :]) ** 2).sum(-1))
    r_, dr_ = rho_drho(kind, phi * d)
    k1 = idx.shape[1]
    eye = np.eye(k1, dtype=dtype)
    both = ok[:, :, None] & ok[:, None, :]
    off = both & ~np.eye(k1, dtype=bool)
    C = np.where(both, s2 * r_ + t2 * eye, eye)
    dS = np.where(both, r_, dtype(0))
    D = np.where(off, s2 * d * dr_, dtype(0))
    dT = np.where(both, eye, dtype(0))
    return C, [dS, D, dT], idx, ok


def rows_bf(coords, nbr, kind, theta, y=None, dtype=np.float64, rows=None):
    """The sweep's form.  Dict of per-row arrays: ``I`` (n, 6), ``G`` (n, 3) (zeros without y), ``logF``, ``q`` =
    r^2 / F."""
    C, dC, idx, ok = blocks(coords, nbr, kind, theta, dtype, rows)
    s2, phi, t2 = (dtype(x) for x in theta)
    n, k = C.shape[0], C.shape[1] - 1
    D = dC[1]
    yy = np.zeros((n, k + 1), dtype) if y is None else np.where(ok, y.astype(dtype)[np.where(ok, idx, 0)], dtype(0))
    L = chol(C[:, :k, :k])
    b = bwd(L, fwd(L, C[:, :k, k:]))[..., 0]
    u = np.concatenate([-b, np.ones((n, 1), dtype)], 1)
    F = np.einsum("na,nab,nb->n", u, C, u)
    nb2 = (b * b).sum(1)
    dF = [(F - t2 * (1 + nb2)) / s2, np.einsum("na,nab,nb->n", u, D, u), 1 + nb2]
    Du = np.einsum("nab,nb->na", D, u)[:, :k]
    sol = fwd(L, np.stack([Du, b, yy[:, :k]], -1))
    w, t, z = sol[..., 0], sol[..., 1], sol[..., 2]
    r = yy[:, k] - (b * yy[:, :k]).sum(1)
    W = [(t2 / s2) * t, w, -t]
    out = {"I": np.zeros((n, 6), dtype), "G": np.zeros((n, 3), dtype), "logF": np.log(F), "q": r * r / F}
    for e, (a, c) in enumerate(TRIU):
        out["I"][:, e] = 0.5 * dF[a] * dF[c] / (F * F) + (W[a] * W[c]).sum(1) / F
    if y is not None:
        for j in range(3):
            out["G"][:, j] = -0.5 * (dF[j] / F) * (1 - r * r / F) + r * (W[j] * z).sum(1) / F
    return out


def rows_trace(coords, nbr, kind, theta, dtype=np.float64, rows=None):
    """The trace-difference form: (n, 6)."""
    C, dC, _, _ = blocks(coords, nbr, kind, theta, dtype, rows)
    k = C.shape[1] - 1
    Ai, Ni = inv(C), inv(C[:, :k, :k])
    PA = [Ai @ d for d in dC]
    PN = [Ni @ d[:, :k, :k] for d in dC]
    out = np.zeros((C.shape[0], 6), dtype)
    for e, (a, c) in enumerate(TRIU):
        out[:, e] = 0.5 * np.einsum("nab,nba->n", PA[a], PA[c]) - 0.5 * np.einsum("nab,nba->n", PN[a], PN[c])
    return out


def dense_info(coords, kind, theta):
    """1/2 tr(K^-1 dK_j K^-1 dK_k) of the dense GP on ``coords``, upper triangle (6,)."""
    n = len(coords)
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))
    r_, dr_ = rho_drho(kind, theta[1] * d)
    K = theta[0] * r_ + theta[2] * np.eye(n)
    D = theta[0] * d * dr_
    np.fill_diagonal(D, 0.0)
    Ki = np.linalg.inv(K)
    P = [Ki @ dK for dK in (r_, D, np.eye(n))]
    return np.array([0.5 * np.trace(P[a] @ P[b]) for a, b in TRIU])


def info3(v6):
    out = np.empty((3, 3))
    for e, (a, c) in enumerate(TRIU):
        out[a, c] = out[c, a] = v6[e]
    return out
