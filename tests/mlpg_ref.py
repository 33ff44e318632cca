"""TEST-ONLY NumPy model of DESIGN.md §12.1: delta rows over runs, the dense matrix W of the delta rule, the trajectory
solve with a dense R and np.linalg.solve (float64) or a dense Cholesky (np.longdouble, which LAPACK does not take), and
the training and conversion of a dynamic map on top of tests/gmm_ref.py.  Runnable in float64 and np.longdouble."""
import numpy as np

import gmm_ref as G

LD = np.longdouble


def runs_of(full):
    """(start, length) int64 arrays of the maximal stretches of True in a bool array."""
    f = np.concatenate(([False], np.asarray(full, dtype=bool), [False]))
    edges = np.flatnonzero(f[1:] != f[:-1])
    return edges[0::2].astype(np.int64), (edges[1::2] - edges[0::2]).astype(np.int64)


def window(span, dtype=np.float64):
    """w_tau, tau = 1 .. span."""
    tau = np.arange(1, span + 1).astype(dtype)
    return tau / (2 * (tau * tau).sum())


def delta_matrix(T, span, dtype=np.float64):
    """W float[T, T]: (W c)_t = sum_tau w_tau (c_clip(t + tau) - c_clip(t - tau)), clip to [0, T - 1]."""
    W = np.zeros((T, T), dtype=dtype)
    for t in range(T):
        for tau, w in enumerate(window(span, dtype), start=1):
            W[t, min(t + tau, T - 1)] += w
            W[t, max(t - tau, 0)] -= w
    return W


def delta_rows(C, span, dtype=np.float64):
    """The delta of every column of C float[n, cols] over the runs of its non-empty rows (column 0 = -inf marks an empty
    row, which gets zeros); tau ascending."""
    C = np.asarray(C, dtype=np.float64)
    out = np.zeros(C.shape, dtype=dtype)
    w = window(span, dtype)
    for s, T in zip(*runs_of(~np.isneginf(C[:, 0]))):
        c = C[s:s + T].astype(dtype)
        idx = np.arange(T)
        acc = np.zeros(c.shape, dtype=dtype)
        for tau in range(1, span + 1):
            acc = acc + w[tau - 1] * (c[np.minimum(idx + tau, T - 1)] - c[np.maximum(idx - tau, 0)])
        out[s:s + T] = acc
    return out


def dynamic_rows(C, span):
    """[c | delta c] float64[n, 2 cols]; an empty row gives (-inf, 0, .. | 0, ..)."""
    C = np.asarray(C, dtype=np.float64)
    return np.hstack((C, delta_rows(C, span)))


def system(P, r, span, d, dtype=np.float64):
    """(R [T, T], q [T]) of column d for one run, both dense: P, r float[T, 2 dy], the static half first.  W^T diag(p) W is
    added row of W by row (each touches a (2 span + 1)-square block of R), which is the same sum in the same order as the
    dense product without its zeros."""
    T, dy = P.shape[0], P.shape[1] // 2
    P, r = np.asarray(P, dtype=np.float64).astype(dtype), np.asarray(r, dtype=np.float64).astype(dtype)
    W = delta_matrix(T, span, dtype)
    R = np.diag(P[:, d])
    for u in range(T):
        lo, hi = max(0, u - span), min(T, u + span + 1)
        R[lo:hi, lo:hi] += P[u, dy + d] * np.outer(W[u, lo:hi], W[u, lo:hi])
    return R, r[:, d] + W.T @ r[:, dy + d]


def dense_solve(R, q):
    if R.dtype == np.float64:
        return np.linalg.solve(R, q)
    L = G.cholesky(R)                                   # long double: LAPACK has none
    n = len(q)
    z = np.zeros(n, dtype=R.dtype)
    for i in range(n):
        z[i] = (q[i] - L[i, :i] @ z[:i]) / L[i, i]
    y = np.zeros(n, dtype=R.dtype)
    for i in range(n - 1, -1, -1):
        y[i] = (z[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
    return y


def solve(P, r, span, run_start, run_len, dtype=np.float64):
    """Y float[n, dy]; rows outside every run are NaN."""
    n, dy = P.shape[0], P.shape[1] // 2
    Y = np.full((n, dy), np.nan, dtype=dtype)
    for s, T in zip(run_start, run_len):
        for d in range(dy):
            R, q = system(P[s:s + T], r[s:s + T], span, d, dtype)
            Y[s:s + T, d] = dense_solve(R, q)
    return Y


# ---- the dynamic map
def select(D, cols, level):
    """The mapped columns of dynamic rows [c | delta c] of `cols` static columns: both halves, without column 0 of each
    unless level."""
    skip = 0 if level else 1
    return np.hstack((D[:, skip:cols], D[:, cols + skip:]))


def train(X, Y, M, level=False, iters=20, tol=1e-5, floor=1e-6, dtype=np.float64):
    """The dynamic map from paired dynamic rows X float64[N, 2 (P + 1)], Y float64[N, 2 (Q + 1)]: gmm_ref.fit's fields
    plus dx, dy (with deltas), A, b, Wx, kx, py in `dtype`."""
    x, y = select(X, X.shape[1] // 2, level), select(Y, Y.shape[1] // 2, level)
    dx = x.shape[1]
    g = G.fit(np.hstack((x, y)), M, iters=iters, tol=tol, floor=floor, split=dx, dtype=dtype)
    mu_c = g["means"] - g["zbar"].astype(dtype)
    A, b, Wx, kx = G.conversion(g["weights"], mu_c, g["covs"], dx)
    S = g["covs"]
    py = np.stack([1 / np.diag(S[m, dx:, dx:] - A[m] @ S[m, :dx, dx:]) for m in range(M)])
    g.update(dx=dx, dy=y.shape[1], level=level, A=A, b=b, Wx=Wx, kx=kx, py=py)
    return g


def trajectory_inputs(g, C, span, dtype=np.float64):
    """(full, P [nf, dy], r [nf, dy], gamma) over the non-empty rows of C for a train() result or a dict of the same fields."""
    C = np.asarray(C, dtype=np.float64)
    dx, level = int(g["dx"]), bool(g["level"])
    full = ~np.isneginf(C[:, 0])
    zbar = np.asarray(g["zbar"]).astype(dtype)
    X = select(np.hstack((C.astype(dtype), delta_rows(C, span, dtype)))[full], C.shape[1], level) - zbar[:dx]
    mu_c = np.asarray(g["means"]).astype(dtype) - zbar
    py, A, b = (np.asarray(g[k]).astype(dtype) for k in ("py", "A", "b"))
    _, _, gamma = G.estep(X, mu_c[:, :dx], np.asarray(g["Wx"]).astype(dtype), np.asarray(g["kx"]).astype(dtype))
    r = G.regress(X, gamma, py[:, :, None] * A, py * (b + zbar[dx:]))
    return full, gamma @ py, r, gamma


def trajectory(g, C, span, dtype=np.float64):
    """conversion_trajectory: float[n, Q + 1] in model_cepstrum's layout."""
    C = np.asarray(C, dtype=np.float64)
    skip = 0 if bool(g["level"]) else 1
    dys = int(g["dy"]) // 2
    full, P, r, _ = trajectory_inputs(g, C, span, dtype)
    out = np.zeros((len(C), dys + skip), dtype=dtype)
    out[~full, 0] = -np.inf
    if full.any():
        start, length = runs_of(full)
        cstart = np.concatenate(([0], np.cumsum(length)[:-1]))
        out[full, skip:] = solve(P, r, span, cstart, length, dtype)
        if skip:
            out[full, 0] = C[full, 0]
    return out


def step_case(T=200, at=100, span=1, p_static=1.0, p_delta=100.0):
    """The step response as a hand-built dynamic map (level=False, order 1 a side: one static column and its delta) and
    its source rows.  Two components: x means -10 and +10 (posteriors one-hot far below rounding), static y means -1 and
    +1, delta means 0, no cross-covariance (A = 0), conditional precisions p_static and p_delta.  The source's c_1 is -10
    before row `at` and +10 from it on.  Returns (conv dict, C float64[T, 2])."""
    means = np.array([[-10.0, 0.0, -1.0, 0.0], [10.0, 0.0, 1.0, 0.0]])
    covs = np.stack([np.diag([1.0, 1e4, 1.0 / p_static, 1.0 / p_delta])] * 2)
    w, zbar = np.array([0.5, 0.5]), np.zeros(4)
    A, b, Wx, kx = G.conversion(w, means - zbar, covs, 2)
    py = np.stack([1.0 / np.diag(covs[m, 2:, 2:] - A[m] @ covs[m, :2, 2:]) for m in range(2)])
    conv = dict(weights=w, means=means, covs=covs, zbar=zbar, phi=np.zeros(4), loglik=np.zeros(1), n=np.int64(T),
                dx=np.int64(2), dy=np.int64(2), level=np.bool_(False), A=A, b=b, Wx=Wx, kx=kx, span=np.int64(span), py=py)
    C = np.zeros((T, 2))
    C[:, 0] = -3.0
    C[:, 1] = np.where(np.arange(T) < at, -10.0, 10.0)
    return conv, C


STEP_ROUGHNESS = 0.19900743719          # the largest adjacent difference of the step case's trajectory


def dynamic_case(N=1500, d=4, M=3, span=2, seed=31):
    """A seeded clustered set with gaps for the end-to-end checks: cepstral rows CA, CB float64[N, d + 1] (column 0 a
    level, the rest gmm_ref.clustered's x and y), the same rows empty in both (runs that touch row 0, single rows, a run
    of two, gaps of one and of many rows, the last row empty), and the paired dynamic rows (X, Y) of the non-empty ones.
    Returns (CA, CB, X, Y, M, span)."""
    x, y, _ = G.clustered(N, d, M, 3.0, 0.3, seed, 1.0)
    rng = np.random.default_rng(seed + 1)
    CA = np.hstack((-4.0 + 0.5 * rng.standard_normal((N, 1)), x))
    CB = np.hstack((-3.0 + 0.5 * rng.standard_normal((N, 1)), y))
    empty = np.zeros(N, dtype=bool)
    for a, b in ((5, 6), (7, 8), (10, 11), (100, 103), (400, 401), (777, 791), (N - 1, N)):
        empty[a:b] = True
    for C in (CA, CB):
        C[empty] = 0.0
        C[empty, 0] = -np.inf
    DA, DB = dynamic_rows(CA, span), dynamic_rows(CB, span)
    return CA, CB, DA[~empty], DB[~empty], M, span
