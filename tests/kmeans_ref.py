"""TEST-ONLY NumPy model of the k-means codebook of DESIGN.md §12.3, written once and runnable in float64 and np.longdouble
(`dtype=`): the assignment, the update, the split rule and the whole loop.  Also the data sets of the tests and the two
rounding bounds they use.

The bound behind decided().  A score is s = g - 2 t, t = z . c a sum of D products, g = |c|^2 a sum of D squares, every
operation rounded once with unit roundoff u = 2^-53.  A sum of D rounded products in any order is within
gamma_D sum_j |z_j c_j| of z . c, gamma_D = D u / (1 - D u) (Higham, Accuracy and Stability of Numerical Algorithms, §3.1;
fused or not, a fused step only drops a rounding); likewise g within gamma_D |g| (its terms are all positive).  The
last operation fma(-2, t, g) rounds once more: a factor (1 + delta), |delta| <= u, on g - 2 t, itself at most
|g| + 2 sum_j |z_j c_j| in modulus.  Together
    |s_computed - s| <= (gamma_D + u + gamma_D u) (|g| + 2 sum_j |z_j c_j|) <= (D + 2) u (|g| + 2 sum_j |z_j c_j|) =: e
for D <= 128.  Two implementations that both obey the bound can order two centres differently only when the exact
scores are within e_a + e_b of each other twice over (each side may err by its own e on both scores): a row is DECIDED
when its second-best score exceeds the best by more than 2 (e_best + e_second), and more than 2 (e_best + e_m) for every
other m as well.

The bound behind sum_bar().  A sum of n terms x_i by n - 1 additions in any order, every addition rounded once, is within
gamma_(n-1) sum |x_i| <= n u sum |x_i| of the exact sum (Higham §4.2); with each term a product z^2 fused into its addition
(Q) the first step rounds as well: n roundings, n u sum z^2 to first order.  The device adds a cluster's rows of a chunk
in order, starting from an exact 0, and then the chunks' sums, again from 0: a cluster of n rows spread over c chunks
takes (n - c) + (c - 1) = n - 1 inexact additions (adding to 0 and adding a chunk's 0 are exact), so the chunks cost
nothing extra.  The bar is twice n u sum |x_i|, n the rows of the cluster; n = 1 leaves S1 exact and Q one rounding."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


# ---- the definition
def rows(Z, split=None, scale=None):
    """(rows float64, zbar, sd): what k-means sees.  Inputs of the iteration, float64 in either precision."""
    Z = np.asarray(Z, dtype=np.float64)
    X = Z[:, :split] if split else Z
    zbar = X.mean(axis=0)
    sd = np.ones(X.shape[1])
    if scale == "std":
        sd = X.std(axis=0)
        sd = np.where(sd > 0, sd, 1.0)
        return (X - zbar) / sd, zbar, sd
    return X - zbar, zbar, sd


def scores(Z, C, dtype=np.float64):
    """s[n, m] = g_m - 2 z_n . c_m; g from the float64 centres in `dtype`."""
    Z, C = np.asarray(Z, dtype=np.float64).astype(dtype), np.asarray(C, dtype=np.float64).astype(dtype)
    return (C * C).sum(axis=1)[None, :] - 2 * (Z @ C.T)


def assign(Z, C, dtype=np.float64):
    """labels int64[N]: the argmin of the scores, the lowest index on equal scores."""
    return np.argmin(scores(Z, C, dtype), axis=1).astype(np.int64)


def decided(Z, C):
    """bool[N]: the rows whose label no implementation within the rounding bound can give differently (module docstring)."""
    Z, C = np.asarray(Z, dtype=np.float64).astype(LD), np.asarray(C, dtype=np.float64).astype(LD)
    D = Z.shape[1]
    s = (C * C).sum(axis=1)[None, :] - 2 * (Z @ C.T)
    e = (D + 2) * LD(U) * ((C * C).sum(axis=1)[None, :] + 2 * (np.abs(Z) @ np.abs(C).T))
    if C.shape[0] == 1:
        return np.ones(len(Z), dtype=bool)
    best = np.argmin(s, axis=1)
    n = np.arange(len(Z))
    gap = s - s[n, best][:, None] - 2 * (e + e[n, best][:, None])
    gap[n, best] = np.inf
    return np.all(gap > 0, axis=1)


def update(Z, labels, K, dtype=np.float64):
    """(count int64[K], S1[K, D], Q[K, D]) in `dtype`; a label outside [0, K) is skipped."""
    Z = np.asarray(Z, dtype=np.float64).astype(dtype)
    count = np.zeros(K, dtype=np.int64)
    S1, Q = np.zeros((K, Z.shape[1]), dtype=dtype), np.zeros((K, Z.shape[1]), dtype=dtype)
    for m in range(K):
        R = Z[labels == m]
        count[m], S1[m], Q[m] = len(R), R.sum(axis=0), (R * R).sum(axis=0)
    return count, S1, Q


def moments(C, count, S1, Q):
    """(centres, v, sse): a cluster without rows keeps its centre and has v = 0, sse = 0."""
    mean, v = np.array(C, dtype=S1.dtype), np.zeros_like(S1)
    for m in range(len(C)):
        if count[m]:
            mean[m] = S1[m] / count[m]
            v[m] = np.maximum(Q[m] / count[m] - mean[m] * mean[m], 0)
    return mean, v, count * v.sum(axis=1)


def split_choice(count, v, sse, k):
    """[(cluster, column)] of a growth step from K = len(count) towards k, in the order the new centres are appended."""
    K = len(count)
    able = [m for m in range(K) if count[m] >= 2 and sse[m] > 0]
    if not able:
        raise np.linalg.LinAlgError("the rows cannot be split further")
    able.sort(key=lambda m: (-sse[m], m))
    return [(m, int(np.argmax(v[m]))) for m in able[:min(K, k - K)]]


def split(C, count, v, sse, k):
    C = np.array(C)
    new = []
    for m, j in split_choice(count, v, sse, k):
        s = np.sqrt(v[m, j])
        c = C[m].copy()
        c[j] += s
        new.append(c)
        C[m, j] -= s
    return np.vstack([C] + new)


def kmeans(R, k, iters=20, split_iters=2, dtype=np.float64):
    """The loop on prepared rows R (rows()): dict(labels, centres (R's coordinates), counts, sse, rounds, sse_history
    [(K, total sse before the round)], assigns [(centres as float64, labels after)] one entry per assignment)."""
    R = np.asarray(R, dtype=np.float64)
    N, D = R.shape
    labels = np.zeros(N, dtype=np.int64)
    C = np.zeros((1, D), dtype=dtype)
    rounds, assigns, hist = 0, [], []

    def do_assign(C):
        C64 = np.asarray(C, dtype=np.float64)          # the centres cross to the device as float64
        lab = assign(R, C64, dtype)
        assigns.append((C64, lab))
        return C64.astype(dtype), lab

    def lloyd(C, labels):
        C, _, sse = moments(C, *update(R, labels, len(C), dtype))
        hist.append((len(C), sse.sum()))
        C, new = do_assign(C)
        return C, new, int((new != labels).sum())
    while len(C) < k:
        count, S1, Q = update(R, labels, len(C), dtype)
        C, v, sse = moments(C, count, S1, Q)
        C, labels = do_assign(split(C, count, v, sse, k))
        for _ in range(split_iters):
            C, labels, _ = lloyd(C, labels)
            rounds += 1
    for _ in range(iters):
        C, labels, changed = lloyd(C, labels)
        rounds += 1
        if changed == 0:
            break
    count, S1, Q = update(R, labels, k, dtype)
    C, _, sse = moments(C, count, S1, Q)
    return dict(labels=labels, centres=C, counts=count, sse=sse, rounds=rounds, sse_history=hist, assigns=assigns)


def sum_bar(R, labels, K):
    """(bar_S1, bar_Q) float64[K, D]: twice the worst-case rounding error of a sum of n_m terms (module docstring)."""
    R = np.asarray(R, dtype=np.float64).astype(LD)
    bS, bQ = np.zeros((K, R.shape[1])), np.zeros((K, R.shape[1]))
    for m in range(K):
        X = R[labels == m]
        n = len(X)
        bS[m] = 2 * n * U * np.abs(X).sum(axis=0).astype(np.float64)
        bQ[m] = 2 * n * U * (X * X).sum(axis=0).astype(np.float64)
    return bS, bQ


# ---- data
def polytope(d, per=100, radius=3.0, sigma=0.5, seed=0):
    """2 d blobs of `per` rows at +- radius e_j in d dimensions, noise sigma, the rows shuffled: float64[2 d per, d]."""
    rng = np.random.default_rng(seed)
    centres = np.vstack((radius * np.eye(d), -radius * np.eye(d)))
    Z = np.repeat(centres, per, axis=0) + sigma * rng.standard_normal((2 * d * per, d))
    return Z[rng.permutation(len(Z))]


# 20 moduli whose squares sum to 63 x 20: with both signs, the noise of one column of one blob of 40 rows
CORNER_NOISE = (0, 2, 1, 2, 2, 3, 3, 4, 4, 5, 6, 6, 7, 8, 9, 11, 11, 12, 14, 18)


def corners(seed=0):
    """8 blobs of 40 rows at the corners (+-31, +-31, +-31) of a cube on an integer grid, in the first three of five
    columns, each column then on a scale and an offset of its own (x 1/4 + 5, x 1/64 - 1, x 2 + 1/4); two columns of noise
    behind; shuffled: float64[320, 5].  For split=3, scale="std".
    Why integers: after scale="std" EVERY column has variance 1, so the first split's column of largest variance is a tie
    that rounding would decide.  Here the noise of a column within a blob is the fixed multiset +-CORNER_NOISE in a seeded
    order: sum 0 and mean square 63, so a column's mean square about its mean is 31^2 + 63 = 1024 = 32^2 times its scale
    squared, every value is a dyadic number of few bits, the mean, the standard deviation, the scaled rows q / 32 and
    every sum of them are exact in any order of addition, and the ties are exact: the lowest index wins in float64, in
    long double and on the device alike."""
    rng = np.random.default_rng(seed)
    sign = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], dtype=np.float64)
    noise = np.array(CORNER_NOISE + tuple(-e for e in CORNER_NOISE), dtype=np.float64)
    q = np.repeat(31.0 * sign, 40, axis=0)
    for blob in range(8):
        for j in range(3):
            q[40 * blob:40 * blob + 40, j] += noise[rng.permutation(40)]
    Z = np.hstack((q * np.array([0.25, 1.0 / 64, 2.0]) + np.array([5.0, -1.0, 0.25]), 0.3 * rng.standard_normal((320, 2))))
    return Z[rng.permutation(320)]


# the separated blobs of the loop tests: name -> (Z, k, split, scale)
def loop_case(name):
    if name == "polytope3":
        return polytope(3, seed=3), 6, None, None
    if name == "corners5":
        return corners(seed=5), 8, 3, "std"
    raise KeyError(name)


def random_case(N, D, K, seed, ldz=None):
    """(Z [N, ldz] with NaN beyond column D, C [K, D]) for the assignment tests: normal rows, centres drawn among the rows
    plus noise, so that scores are close enough to matter and far enough to be decided."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    C = X[rng.integers(0, N, size=K)] + 0.5 * rng.standard_normal((K, D))
    Z = np.full((N, ldz or D), np.nan)
    Z[:, :D] = X
    return Z, C


# (N, D, K, ldz): every edge of the k-step of 4, of the 16-wide panels and of the 64-row block, not the full product
ASSIGN_SHAPES = (
    (1, 1, 1, None), (63, 3, 2, None), (64, 4, 15, None), (65, 5, 16, 7), (129, 16, 17, None), (129, 17, 63, 20),
    (65, 64, 64, None), (63, 127, 17, 128), (129, 128, 64, None), (64, 1, 64, 3), (1, 128, 2, None), (129, 5, 1, None),
)


def assign_case(i):
    N, D, K, ldz = ASSIGN_SHAPES[i]
    return random_case(N, D, K, 100 + i, ldz)


def tie_case():
    """Small integers: every product, sum and score is exact, so the device must give the exact argmin with the lowest
    index on every tie.  40 centres in 20 columns; 3 = 20 and 5 = 37 are identical centres in different panels of 16;
    38 and 39 are alone far out on column 0 with row 0 half way between them."""
    rng = np.random.default_rng(7)
    C = rng.integers(-3, 4, size=(40, 20)).astype(np.float64)
    C[20], C[37] = C[3], C[5]
    C[38], C[39] = 0.0, 0.0
    C[38, 0], C[39, 0] = 100.0, 104.0
    Z = rng.integers(-3, 4, size=(130, 20)).astype(np.float64)
    Z[0] = 0.0
    Z[0, 0] = 102.0
    Z[1:41] = C                                                     # a copy of every centre: the identical ones tie
    Z[41:81] = C + rng.integers(-1, 2, size=(40, 20))
    return Z, C


def update_case(N, D, Kc, seed, empty=None, stray=False):
    rng = np.random.default_rng(seed)
    Z = 2.0 + rng.standard_normal((N, D)) * np.linspace(0.5, 3.0, D)
    labels = rng.integers(0, Kc, size=N)
    if empty is not None:
        labels[labels == empty] = (empty + 1) % Kc
    if stray:
        labels[::97] = Kc
        labels[5::101] = -1
    return Z, labels


# N = the chunk (512 rows up to N = 65536) -1, +0, +1 and two chunks + 1; an empty cluster; K = 64; D = 128; labels
# outside [0, K)
UPDATE_CASES = [(511, 5, 3, 1, False), (512, 17, 4, None, False), (513, 3, 64, None, False), (1025, 128, 2, None, False),
                (1025, 36, 8, 5, True), (70, 128, 64, 0, False)]
