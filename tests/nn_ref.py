"""TEST-ONLY NumPy model of the nearest-row search and of the non-parallel training loop of DESIGN.md §12.5, written once
and runnable in float64 and np.longdouble (`dtype=`).  Also the data sets of the tests and the bound on dist2.

The score is the k-means assignment's with B as the centres, s_ij = |b_j|^2 - 2 a_i . b_j, and so is its rounding bound:
decided() IS kmeans_ref.decided (its docstring derives the bound), imported, not copied.

The bound behind dist2_bar().  dist2 = sum_k (a_k - b_k)^2, every difference rounded once, d_k (1 + e_k), |e_k| <= u =
2^-53, its square fused into the sum: one more rounding per column, D in all, on a sum of non-negative terms.  Squaring
the rounded difference gives d_k^2 (1 + e_k)^2, and a sum of D non-negative terms by D rounded (fused) steps is within
gamma_D of itself (Higham, Accuracy and Stability of Numerical Algorithms, §3.1, §4.2); together
    |computed - exact| <= ((1 + u)^2 (1 + gamma_D) - 1) exact <= (D + 2) u exact + O(u^2):
D + 1 roundings in the issue's count (the difference's counts twice, to first order 2 u).  The bar of the tests is twice
(D + 2) u times the exact value: it is 0 for equal rows, so dist2 must be exactly 0 there."""
import math

import numpy as np

import gmm_ref as G
from kmeans_ref import decided  # noqa: F401  (the same score, the same bound: B are the centres)

LD = np.longdouble
U = 2.0 ** -53


# ---- the definition
def scores(A, B, dtype=np.float64):
    """s[i, j] = |b_j|^2 - 2 a_i . b_j in `dtype`, from float64 rows."""
    A, B = np.asarray(A, dtype=np.float64).astype(dtype), np.asarray(B, dtype=np.float64).astype(dtype)
    return (B * B).sum(axis=1)[None, :] - 2 * (A @ B.T)


def nearest(A, B, dtype=np.float64):
    """index int64[nA]: the argmin of the scores, the lowest index on equal scores."""
    return np.argmin(scores(A, B, dtype), axis=1).astype(np.int64)


def dist2(A, B, index, dtype=np.float64):
    """dist2[i] = |a_i - b_index[i]|^2 in `dtype`, from the rows themselves."""
    A, B = np.asarray(A, dtype=np.float64).astype(dtype), np.asarray(B, dtype=np.float64).astype(dtype)
    d = A - B[index]
    return (d * d).sum(axis=1)


def dist2_bar(A, B, index):
    """float64[nA]: twice the worst-case rounding error (D + 2) u dist2 of the device's dist2 (module docstring)."""
    D = np.asarray(A).shape[1]
    return 2 * (D + 2) * U * dist2(A, B, index, LD).astype(np.float64)


def within_bound(A, B, index):
    """bool[nA]: the exact (long-double) score of the choice `index` is within the decision bound of the best score, 2 (e +
    e_best) with kmeans_ref's e = (D + 2) u (|b|^2 + 2 |a| . |b|): what an implementation that obeys the rounding bound may
    choose on a row that is not decided."""
    A, B = np.asarray(A, dtype=np.float64).astype(LD), np.asarray(B, dtype=np.float64).astype(LD)
    D = A.shape[1]
    g = (B * B).sum(axis=1)
    s = g[None, :] - 2 * (A @ B.T)
    e = (D + 2) * LD(U) * (g[None, :] + 2 * (np.abs(A) @ np.abs(B).T))
    n, best = np.arange(len(A)), np.argmin(s, axis=1)
    return s[n, index] - s[n, best] <= 2 * (e[n, index] + e[n, best])


def pairs(p, q=None):
    """The pairs of one round, int64[L, 2]: (k, p_k) and, with q, (q_j, j); duplicates dropped, sorted by (k, j)."""
    out = {(k, int(j)) for k, j in enumerate(p)}
    if q is not None:
        out |= {(int(k), j) for j, k in enumerate(q)}
    return np.array(sorted(out), dtype=np.int64).reshape(-1, 2)


def loop(X, Y, components, rounds=8, tol=1e-3, symmetric=True, iters=20, em_tol=1e-5, floor=1e-6, dtype=np.float64,
         init_split=True):
    """The loop of §12.5 with every column mapped (level=True) on rows without empty ones, gmm_ref's fit and convert in
    `dtype`: dict(trace [r_stop + 1], fits [gmm_ref.fit results], pairs [int64[L, 2] per trained map], xc [the rows each
    search started from], best).  init_split: initialise on the x columns only, as conversion_train does."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    dx = X.shape[1]
    xc = X
    trace, fits, prs, xcs = [], [], [], []
    while True:
        xcs.append(xc)
        p = nearest(xc, Y, dtype)
        dp = dist2(xc, Y, p, dtype)
        q = None
        if symmetric:
            q = nearest(Y, xc, dtype)
            dq = dist2(Y, xc, q, dtype)
            tr = (fsum(dp) + fsum(dq)) / (len(X) + len(Y))
        else:
            tr = fsum(dp) / len(X)
        trace.append(tr)
        r = len(trace) - 1
        if (r >= 1 and trace[r] > (1 - tol) * trace[r - 1]) or r == rounds:
            break
        pr = pairs(p, q)
        fit = G.fit(np.hstack((X[pr[:, 0]], Y[pr[:, 1]])), components, iters=iters, tol=em_tol, floor=floor,
                    split=dx if init_split else None, dtype=dtype)
        fits.append(fit)
        prs.append(pr)
        # the converted rows cross to the next search as float64, as they do from the device
        xc = np.asarray(G.convert(fit, dx, X), dtype=np.float64)
    best = 1 + int(np.argmin(np.array(trace[1:], dtype=np.float64)))
    return dict(trace=np.array(trace, dtype=dtype), fits=fits, pairs=prs, xc=xcs, best=best)


def fsum(v):
    return math.fsum(float(x) for x in v) if v.dtype == np.float64 else v.sum()


def rms(a, b):
    """The root of the mean squared difference over all entries."""
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)))


# ---- data
def inca_set(N=2400, d=3, M=6, seed=11):
    """The set of DESIGN.md §12.5: M cluster centres 3 randn; x = mu_m + 0.4 randn; y = mu_m + A_m (x - mu_m) + b_m +
    0.05 randn, A_m = I + 0.3 randn, b_m = 0.5 randn; drawn in the order mu, labels, x-noise, A, b, y-noise.  Split in
    thirds by position: (x of the first third, y of the SECOND third) train, not parallel; the last third's pairs are
    held out.  Returns dict(X, Y, Xtrue, Ytrue (the first third's true pairs), Xh, Yh)."""
    rng = np.random.default_rng(seed)
    mu = 3 * rng.standard_normal((M, d))
    lab = rng.integers(0, M, size=N)
    x = mu[lab] + 0.4 * rng.standard_normal((N, d))
    A = np.eye(d)[None] + 0.3 * rng.standard_normal((M, d, d))
    b = 0.5 * rng.standard_normal((M, d))
    y = mu[lab] + np.einsum("nij,nj->ni", A[lab], x - mu[lab]) + b[lab] + 0.05 * rng.standard_normal((N, d))
    t = N // 3
    return dict(X=x[:t], Y=y[t:2 * t], Xtrue=x[:t], Ytrue=y[:t], Xh=x[2 * t:], Yh=y[2 * t:], components=M)


def random_case(nA, nB, D, seed, lda=None, ldb=None):
    """(A [nA, lda], B [nB, ldb]) with NaN beyond column D: normal rows of B, the rows of A drawn among them plus noise,
    so that scores are close enough to matter and far enough to be decided."""
    rng = np.random.default_rng(seed)
    Bx = rng.standard_normal((nB, D))
    Ax = Bx[rng.integers(0, nB, size=nA)] + 0.5 * rng.standard_normal((nA, D))
    A, B = np.full((nA, lda or D), np.nan), np.full((nB, ldb or D), np.nan)
    A[:, :D], B[:, :D] = Ax, Bx
    return A, B


# (nA, nB, D, lda, ldb): every edge of the k-step of 4, of the 16-row tiles, of the 64-row block and panel and of the
# split, not the full product.  4160 = 65 panels in 2 splits; 8200 is no multiple of the panel, 3 splits.
SEARCH_SHAPES = (
    (1, 1, 1, None, None), (15, 16, 3, None, None), (16, 17, 4, 6, 5), (17, 63, 5, None, None), (63, 64, 36, 40, 36),
    (64, 65, 127, 128, 130), (65, 129, 128, None, None), (130, 129, 128, 131, 129), (130, 4160, 5, None, 7),
    (65, 8200, 36, 37, None), (17, 8200, 128, None, None), (1, 4160, 1, 2, 2),
)


def search_case(i):
    nA, nB, D, lda, ldb = SEARCH_SHAPES[i]
    return random_case(nA, nB, D, 200 + i, lda, ldb)


def tie_case():
    """Small integers: every product, sum and score is exact, so the device must give the exact argmin with the lowest
    index on every tie.  B has 8200 rows of 6 columns (3 splits: panels 0..42, 43..85, 86..128, rows 0..2751, 2752..5503,
    5504..8199), all far out (column 0 at 1000 or beyond) except the planted ones near the origin:
      5 = 40      identical rows within one panel
      60 = 70     identical rows across a panel boundary
      2700 = 2800 identical rows across the first split boundary
      100, 6000   two different rows at the same distance from row 3 of A, in different splits
    A has 70 rows: a copy of each planted row (dist2 exactly 0), a row half way between rows 100 and 6000, and small
    integers around them."""
    rng = np.random.default_rng(17)
    B = rng.integers(-3, 4, size=(8200, 6)).astype(np.float64)
    B[:, 0] += 1000.0 + np.arange(8200) % 7
    planted = {5: 0, 40: 0, 60: 1, 70: 1, 2700: 2, 2800: 2}
    P = rng.integers(-3, 4, size=(3, 6)).astype(np.float64)
    P[1, 1], P[2, 2] = 9.0, -9.0                                    # three distinct points
    for j, m in planted.items():
        B[j] = P[m]
    B[100], B[6000] = 0.0, 0.0
    B[100, 5], B[6000, 5] = 20.0, 24.0
    A = rng.integers(-3, 4, size=(70, 6)).astype(np.float64)
    A[0], A[1], A[2] = P[0], P[1], P[2]
    A[3] = 0.0
    A[3, 5] = 22.0
    want = {0: 5, 1: 60, 2: 2700, 3: 100}
    return A, B, want
