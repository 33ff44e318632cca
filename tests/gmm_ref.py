"""TEST-ONLY NumPy model of the joint-density Gaussian mixture of DESIGN.md §12, written once and runnable in float64
and np.longdouble (`dtype=`).  The Cholesky factor and the triangular inverse are vectorised by rows, so that D = 128 in
long double takes a fraction of a second.  Also the data sets of the tests: clusters in x, one affine map per cluster
to y, noise on y."""
import math

import numpy as np

LD = np.longdouble


# ---- small algebra in any dtype
def cholesky(A):
    """Lower L with L L^T = A, column by column; LinAlgError when a pivot is not > 0."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive" % j)
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def tri_inverse(L):
    """W = L^-1 for lower-triangular L, row by row: W[i] = (e_i - L[i, :i] W[:i]) / L[i, i]."""
    n = L.shape[0]
    W = np.zeros_like(L)
    for i in range(n):
        row = -(L[i, :i] @ W[:i]) if i else np.zeros(n, dtype=L.dtype)
        row[i] += 1
        W[i] = row / L[i, i]
    return W


# ---- the definition
def centre(Z, floor=1e-6, dtype=np.float64):
    """(zbar float64[D], c = Z - zbar in `dtype`, phi float64[D]).  zbar and phi are the host's float64 numbers in
    either precision: they are inputs of the iteration, not part of it.  var is the population variance (ddof = 0)."""
    Z = np.asarray(Z, dtype=np.float64)
    zbar = Z.mean(axis=0)
    c64 = Z - zbar
    phi = floor * c64.var(axis=0)
    return zbar, (Z.astype(dtype) - zbar.astype(dtype)), phi


def init_labels(X, M):
    """The default initialisation: labels int64[N] from the rank of the projection of the standardised columns of X on
    the principal axis of their covariance."""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    sd = X.std(axis=0)
    U = (X - X.mean(axis=0)) / np.where(sd > 0, sd, 1.0)
    cov = U.T @ U / N
    _, vec = np.linalg.eigh(cov)
    axis = vec[:, -1]
    if axis[np.argmax(np.abs(axis))] < 0:
        axis = -axis
    order = np.argsort(U @ axis, kind="stable")
    labels = np.empty(N, dtype=np.int64)
    labels[order] = np.arange(N, dtype=np.int64) * M // N
    return labels


def one_hot(labels, M, dtype=np.float64):
    g = np.zeros((len(labels), M), dtype=dtype)
    g[np.arange(len(labels)), labels] = 1
    return g


def sufficient(c, gamma):
    """(S0 [M], S1 [M, D], S2 [M, D, D]) in c's dtype."""
    S0 = gamma.sum(axis=0)
    S1 = gamma.T @ c
    S2 = np.stack([(c * gamma[:, m:m + 1]).T @ c for m in range(gamma.shape[1])])
    low = np.tril(S2)
    return S0, S1, low + np.tril(S2, -1).transpose(0, 2, 1)      # exactly symmetric: the upper triangle is a copy


def finish_mstep(S0, S1, S2, N, phi):
    """(w, mu, Sigma) from the sums; LinAlgError naming the component whose S0 < 1."""
    if np.any(S0 < 1):
        raise np.linalg.LinAlgError("component %d is starved: its responsibilities sum to %.3g < 1"
                                    % (int(np.flatnonzero(S0 < 1)[0]), float(S0[S0 < 1][0])))
    w = S0 / N
    mu = S1 / S0[:, None]
    Sigma = S2 / S0[:, None, None] - mu[:, :, None] * mu[:, None, :]
    Sigma = Sigma + np.diag(phi.astype(S0.dtype))[None]
    return w, mu, Sigma


def mstep(c, gamma, phi):
    return finish_mstep(*sufficient(c, gamma), c.shape[0], phi)


def estep_parameters(w, mu, Sigma):
    """(W [M, D, D], k [M]) of the E-step; LinAlgError naming the component whose Cholesky breaks down."""
    M, D = mu.shape
    W = np.zeros_like(Sigma)
    k = np.zeros(M, dtype=Sigma.dtype)
    two_pi = Sigma.dtype.type(8) * np.arctan(Sigma.dtype.type(1))
    for m in range(M):
        try:
            L = cholesky(Sigma[m])
        except np.linalg.LinAlgError as e:
            raise np.linalg.LinAlgError("the covariance of component %d is not positive definite (%s)" % (m, e)) from None
        W[m] = tri_inverse(L)
        k[m] = np.log(w[m]) - (D * np.log(two_pi) + 2 * np.log(np.diag(L)).sum()) / 2
    return W, k


def estep(c, mu, W, k):
    """(lp [N, M], ll [N], gamma [N, M])."""
    N, M = c.shape[0], mu.shape[0]
    lp = np.empty((N, M), dtype=c.dtype)
    for m in range(M):
        y = (c - mu[m]) @ W[m].T
        lp[:, m] = k[m] - (y * y).sum(axis=1) / 2
    mx = lp.max(axis=1)
    ll = mx + np.log(np.exp(lp - mx[:, None]).sum(axis=1))
    return lp, ll, np.exp(lp - ll[:, None])


def mean_loglik(ll):
    return math.fsum(float(v) for v in ll) / len(ll) if ll.dtype == np.float64 else ll.sum() / len(ll)


def fit(Z, M, iters=20, tol=1e-5, floor=1e-6, init=None, split=None, dtype=np.float64):
    """The loop of §12: dict(weights, means (un-centred), covs, zbar, phi, loglik, n and the last E-step's gamma, ll)
    in `dtype`."""
    Z = np.asarray(Z, dtype=np.float64)
    N = Z.shape[0]
    zbar, c, phi = centre(Z, floor, dtype)
    labels = init_labels(Z[:, :split] if split else Z, M) if init is None else np.asarray(init, dtype=np.int64)
    w, mu, Sigma = mstep(c, one_hot(labels, M, dtype), phi)
    loglik, gamma, ll = [], None, None
    for _ in range(iters):
        W, k = estep_parameters(w, mu, Sigma)
        _, ll, gamma = estep(c, mu, W, k)
        loglik.append(mean_loglik(ll))
        if len(loglik) > 1 and loglik[-1] - loglik[-2] < tol:
            break
        w, mu, Sigma = mstep(c, gamma, phi)
    return dict(weights=w, means=mu + zbar.astype(dtype), covs=Sigma, zbar=zbar, phi=phi,
                loglik=np.array(loglik, dtype=dtype), n=N, gamma=gamma, ll=ll)


def conversion(w, mu_c, Sigma, dx):
    """(A [M, dy, dx], b [M, dy] on centred coordinates, Wx [M, dx, dx], kx [M]) from centred means."""
    M = len(w)
    Wx, kx = estep_parameters(w, mu_c[:, :dx], Sigma[:, :dx, :dx])
    A = np.stack([Sigma[m, dx:, :dx] @ Wx[m].T @ Wx[m] for m in range(M)])      # Sigma_yx Sigma_xx^-1
    b = mu_c[:, dx:] - np.einsum("mij,mj->mi", A, mu_c[:, :dx])
    return A, b, Wx, kx


def regress(xc, gamma, A, b):
    """yhat on centred coordinates: sum_m gamma_nm (b_m + A_m x_n)."""
    return np.einsum("nm,nmi->ni", gamma, b[None] + np.einsum("mij,nj->nmi", A, xc))


def convert(g, dx, X):
    """The conversion of rows X [n, dx] by a fit() result: float [n, dy]."""
    zbar = g["zbar"].astype(g["means"].dtype)
    mu_c = g["means"] - zbar
    A, b, Wx, kx = conversion(g["weights"], mu_c, g["covs"], dx)
    xc = np.asarray(X, dtype=np.float64).astype(mu_c.dtype) - zbar[:dx]
    _, _, gamma = estep(xc, mu_c[:, :dx], Wx, kx)
    return regress(xc, gamma, A, b) + zbar[dx:]


# ---- data: clusters in x, one affine map per cluster to y
def clustered(N, d, M, spread, sigma, seed, offset=3.0):
    """(X [N, d], Y [N, d], labels): cluster centres at least `spread` standard deviations apart (unit-variance clusters), a
    random affine map per cluster with offsets of scale `offset`, noise sigma on y."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((M, d))
    centres = spread * np.arange(M)[:, None] * u / np.sqrt((u ** 2).sum(axis=1))[:, None]   # |c_m - c_m'| >= spread |m - m'|
    labels = rng.integers(0, M, size=N)
    labels[:M] = np.arange(M)
    X = centres[labels] + rng.standard_normal((N, d))
    maps = rng.standard_normal((M, d, d)) / np.sqrt(d)
    offs = offset * rng.standard_normal((M, d))
    Y = np.einsum("nij,nj->ni", maps[labels], X) + offs[labels] + sigma * rng.standard_normal((N, d))
    return X, Y, labels


# the data sets of the issue's table: (name, N, d, M, spread, noise on y, offset scale, seed).  Well separated: centres 8
# standard deviations apart, noise 0.05.  Overlapping: centres 1.5 apart, maps close to each other and noise 0.5, so
# that the joint clusters overlap as well and the responsibilities are soft.
SIGMA = 0.05
CASES = (
    ("sep_600x3", 600, 3, 3, 8.0, SIGMA, 3.0, 11),
    ("sep_1500x8", 1500, 8, 4, 8.0, SIGMA, 3.0, 12),
    ("ovl_700x3", 700, 3, 3, 1.5, 0.5, 0.5, 13),
    ("ovl_1500x8", 1500, 8, 4, 1.5, 0.5, 0.5, 14),
    ("ovl_257x1", 257, 1, 2, 0.5, 0.5, 0.2, 15),
    ("sep_400x64", 400, 64, 2, 8.0, SIGMA, 3.0, 16),
)


def case(name):
    """(X, Y, labels, M) of a named data set."""
    for nm, N, d, M, spread, sigma, offset, seed in CASES:
        if nm == name:
            X, Y, labels = clustered(N, d, M, spread, sigma, seed, offset)
            return X, Y, labels, M
    raise KeyError(name)
