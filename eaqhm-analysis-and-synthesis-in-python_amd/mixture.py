"""Rows in, clusters out: the k-means codebook and the Gaussian mixture on the device (not in the reference).  Nothing
here knows of cepstra or maps; the first layer below convert.

    gmm_fit(Z, components, *, iters=20, tol=1e-5, floor=1e-6, init=None, split=None, device_index=0)
        -> dict(weights[M], means[M, D], covs[M, D, D], zbar[D], phi[D], loglik[n_E_steps], n)
    gmm_posteriors(gmm, Z, *, device_index=0) -> (gamma[N, M], ll[N])
    kmeans(Z, k, *, iters=20, split_iters=2, split=None, scale=None, device_index=0)
        -> dict(labels int64[N], centres[k, D'], counts int64[k], sse[k], rounds)
    kmeans_assign(centres, Z, *, device_index=0) -> int64[N]
    check_gmm_arguments, check_kmeans_arguments, check_gmm: validation, no device work
    gmm_centre, gmm_init_labels, gmm_finish_mstep, gmm_estep_parameters: the mixture's host algebra
    kmeans_rows, kmeans_moments, kmeans_split, kmeans_grow: the codebook's host side
    gmm_chunk_rows, gmm_work_len, kmeans_work_len: host mirrors of the library's buffer sizes
    _Mixture, _Codebook: the rows of one fit on the device and the buffers of its steps

The two stay in one module: the codebook's work buffer is sized by the M-step's chunk rule, and gmm_fit(init="kmeans")
grows a codebook (_kmeans_responsibilities).  Everything that scales with the number of rows runs in libeaqhm_hip.so
(eaqhm_gmm_estep, eaqhm_gmm_mstep, eaqhm_kmeans_assign, eaqhm_kmeans_update); the per-component algebra and the split
decisions are host NumPy.  There is no CPU path.
"""
import math

import numpy as np

from .args import _integer, _real, _rows
from .records import _agree, _device

GMM_MAX_COLUMNS = 128      # D = dx + dy at most: nine 16-wide tile rows of [c | 1] in the M-step's registers
GMM_MAX_SIDE = 64          # dx, dy at most
GMM_MAX_COMPONENTS = 64
GMM_FLOOR_RANGE = (1e-12, 1e-1)
GMM_MAX_ITERS = 1000
GMM_CHUNK_MIN = 512        # rows of an M-step chunk at least
GMM_CHUNKS_MAX = 128       # chunks at most
KMEANS_MAX_CENTRES = 64
KMEANS_MAX_ITERS = 1000
KMEANS_MAX_SPLIT_ITERS = 100
KMEANS_START = dict(iters=20, split_iters=2)   # the codebook behind init="kmeans": kmeans' own defaults


def gmm_chunk_rows(N):
    """Rows per chunk of the M-step (include/eaqhm_hip.h): max(512, 64 ceil(ceil(N / 128) / 64)), a function of N alone."""
    per = -(-int(N) // GMM_CHUNKS_MAX)
    return max(GMM_CHUNK_MIN, -(-per // 64) * 64)


def gmm_work_len(N, D, M):
    """Doubles of the M-step's `work`: ceil(N / R) M T 256, T the lower-triangle 16 x 16 tiles of D + 1 columns."""
    nt = (D + 1 + 15) // 16
    return -(-int(N) // gmm_chunk_rows(N)) * M * (nt * (nt + 1) // 2) * 256


def kmeans_work_len(N, D, K):
    """Doubles of the k-means update's `work` (include/eaqhm_kmeans.h): ceil(N / R) K (2 D + 1), R the M-step's chunk."""
    return -(-int(N) // gmm_chunk_rows(N)) * K * (2 * D + 1)


# ---- validation (no device work)
def check_gmm_arguments(Z, components, iters=20, tol=1e-5, floor=1e-6, init=None, split=None):
    """Validates everything gmm_fit gets (no device work): returns (Z float64[N, D], M, iters, tol, floor, init, split),
    init an int64[N] of labels, "kmeans" or None."""
    Z = _rows(Z, "Z", GMM_MAX_COLUMNS)
    N, D = Z.shape
    M = _integer(components, "components")
    if not 1 <= M <= GMM_MAX_COMPONENTS:
        raise ValueError("components must be in [1, %d], got %d" % (GMM_MAX_COMPONENTS, M))
    if N < 2 * M:
        raise ValueError("%d components need at least %d rows, got %d" % (M, 2 * M, N))
    iters = _integer(iters, "iters")
    if not 1 <= iters <= GMM_MAX_ITERS:
        raise ValueError("iters must be in [1, %d], got %d" % (GMM_MAX_ITERS, iters))
    tol = _real(tol, "tol", 0.0, np.inf)
    if not np.isfinite(tol):
        raise ValueError("tol must be finite")
    floor = _real(floor, "floor", *GMM_FLOOR_RANGE)
    if isinstance(init, str):
        if init != "kmeans":
            raise ValueError('init must be None, "kmeans" or an integer array of labels, got %r' % init)
    elif init is not None:
        lab = np.asarray(init)
        if lab.dtype.kind not in "iu" or lab.shape != (N,):
            raise ValueError("init must be an integer array of %d labels, one per row" % N)
        lab = lab.astype(np.int64)
        if lab.min() < 0 or lab.max() >= M:
            raise ValueError("init labels must be in [0, %d)" % M)
        count = np.bincount(lab, minlength=M)
        if np.any(count == 0):
            raise ValueError("init leaves component %d without a row" % int(np.flatnonzero(count == 0)[0]))
        init = lab
    if split is not None:
        split = _integer(split, "split")
        if not 1 <= split <= D:
            raise ValueError("split must be in [1, %d], got %d" % (D, split))
    return Z, M, iters, tol, floor, init, split


def check_kmeans_arguments(Z, k, iters=20, split_iters=2, split=None, scale=None):
    """Validates everything kmeans gets (no device work): returns (Z float64[N, D], k, iters, split_iters, split, scale)."""
    Z = _rows(Z, "Z", GMM_MAX_COLUMNS)
    N, D = Z.shape
    k = _integer(k, "k")
    if not 1 <= k <= KMEANS_MAX_CENTRES:
        raise ValueError("k must be in [1, %d], got %d" % (KMEANS_MAX_CENTRES, k))
    if N < 2 * k:
        raise ValueError("%d centres need at least %d rows, got %d" % (k, 2 * k, N))
    iters = _integer(iters, "iters")
    if not 0 <= iters <= KMEANS_MAX_ITERS:
        raise ValueError("iters must be in [0, %d], got %d" % (KMEANS_MAX_ITERS, iters))
    split_iters = _integer(split_iters, "split_iters")
    if not 0 <= split_iters <= KMEANS_MAX_SPLIT_ITERS:
        raise ValueError("split_iters must be in [0, %d], got %d" % (KMEANS_MAX_SPLIT_ITERS, split_iters))
    if split is not None:
        split = _integer(split, "split")
        if not 1 <= split <= D:
            raise ValueError("split must be in [1, %d], got %d" % (D, split))
    if scale is not None and not (isinstance(scale, str) and scale == "std"):
        raise ValueError('scale must be None or "std", got %r' % (scale,))
    return Z, k, iters, split_iters, split, scale


def _field(conv, name, shape=None):
    try:
        a = np.asarray(conv[name])
    except (KeyError, TypeError, IndexError):
        raise ValueError("the conversion lacks the field %r" % name) from None
    if a.dtype.kind not in "iufb":
        raise ValueError("the conversion's %s must be numbers" % name)
    if shape is not None and a.shape != shape:
        raise ValueError("the conversion's %s must have shape %s, got %s" % (name, shape, a.shape))
    if not np.all(np.isfinite(a)):
        raise ValueError("the conversion's %s must be finite" % name)
    return a


def check_gmm(gmm):
    """Validates a mixture dict (gmm_fit's, or one loaded from a file): shapes, finiteness, positive weights that sum to 1
    within 1e-9, symmetric covariances with a positive diagonal.  Returns (weights, means, covs, zbar) as float64."""
    w = _field(gmm, "weights").astype(np.float64)
    if w.ndim != 1 or not 1 <= len(w) <= GMM_MAX_COMPONENTS:
        raise ValueError("the mixture's weights must be a 1-D array of 1 to %d entries" % GMM_MAX_COMPONENTS)
    M = len(w)
    mu = _field(gmm, "means").astype(np.float64)
    if mu.ndim != 2 or mu.shape[0] != M or not 1 <= mu.shape[1] <= GMM_MAX_COLUMNS:
        raise ValueError("the mixture's means must have shape (%d, D), 1 <= D <= %d" % (M, GMM_MAX_COLUMNS))
    D = mu.shape[1]
    S = _field(gmm, "covs", (M, D, D)).astype(np.float64)
    zbar = _field(gmm, "zbar", (D,)).astype(np.float64)
    if np.any(w <= 0) or abs(math.fsum(w) - 1.0) > 1e-9:
        raise ValueError("the mixture's weights must be positive and sum to 1 within 1e-9")
    if not np.array_equal(S, S.transpose(0, 2, 1)):
        raise ValueError("the mixture's covariances must be symmetric")
    if np.any(np.einsum("mii->mi", S) <= 0):
        raise ValueError("the mixture's covariances must have a positive diagonal")
    return w, mu, S, zbar


# ---- host algebra (float64)
def gmm_centre(Z, floor):
    """(zbar, phi): the mean of the rows and the covariance floor, floor x the population variance of each column."""
    zbar = Z.mean(axis=0)
    return zbar, floor * (Z - zbar).var(axis=0)


def gmm_init_labels(X, M):
    """The default initialisation: standardise the columns, project on the principal axis of their covariance (sign: the
    component of largest modulus positive), stable-sort, cut into M runs of equal count: the row of rank r gets r M // N."""
    N = X.shape[0]
    sd = X.std(axis=0)
    U = (X - X.mean(axis=0)) / np.where(sd > 0, sd, 1.0)
    _, vec = np.linalg.eigh(U.T @ U / N)
    axis = vec[:, -1]
    if axis[np.argmax(np.abs(axis))] < 0:
        axis = -axis
    order = np.argsort(U @ axis, kind="stable")
    labels = np.empty(N, dtype=np.int64)
    labels[order] = np.arange(N, dtype=np.int64) * M // N
    return labels


def kmeans_rows(Z, split=None, scale=None):
    """(rows, zbar, sd): the rows k-means sees, the first `split` columns of Z minus their mean and,
    with scale="std", over their standard deviations (a constant column is left as it is); sd is ones without."""
    X = Z[:, :split] if split else Z
    zbar = X.mean(axis=0)
    sd = np.ones(X.shape[1])
    if scale:
        sd = X.std(axis=0)
        sd = np.where(sd > 0, sd, 1.0)
    return np.ascontiguousarray((X - zbar) / sd if scale else X - zbar), zbar, sd


def kmeans_moments(C, count, S1, Q):
    """(centres, v, sse) from the sums of an update: the means S1 / n, the per-column variances max(Q / n - mean^2, 0) and
    n sum_j v_j; a cluster without a row keeps its centre of `C` and has v = 0, sse = 0."""
    full = (count > 0)[:, None]
    n = np.maximum(count, 1)[:, None].astype(np.float64)
    mean = np.where(full, S1 / n, C)
    v = np.where(full, np.maximum(Q / n - mean * mean, 0.0), 0.0)
    return mean, v, count * v.sum(axis=1)


def kmeans_split(C, count, v, sse, k):
    """Grows K = len(C) centres towards k: the min(K, k - K) clusters of largest sse among those with n >= 2 and sse > 0
    (ties: the lower index first) are split, in that order, along their column j of largest variance (ties: the lowest):
    the new centre c + sqrt(v_j) e_j is appended and the old one becomes c - sqrt(v_j) e_j.  LinAlgError when no cluster
    qualifies."""
    K = len(C)
    able = np.flatnonzero((count >= 2) & (sse > 0))
    if not len(able):
        raise np.linalg.LinAlgError("k-means: the rows cannot be split further than %d centres (%d wanted): every cluster "
                                    "is a single point" % (K, k))
    chosen = able[np.argsort(-sse[able], kind="stable")][:min(K, k - K)]
    C = np.vstack((C, C[chosen]))
    for i, m in enumerate(chosen):
        j = int(np.argmax(v[m]))
        s = math.sqrt(v[m, j])
        C[K + i, j] += s
        C[m, j] -= s
    return C


def gmm_finish_mstep(S0, S1, S2, N, phi):
    """(w, mu, Sigma) from the sums; LinAlgError naming the component whose S0 < 1: there is no re-seeding."""
    if np.any(S0 < 1):
        m = int(np.flatnonzero(S0 < 1)[0])
        raise np.linalg.LinAlgError("component %d is starved: its responsibilities sum to %.3g < 1" % (m, S0[m]))
    mu = S1 / S0[:, None]
    Sigma = S2 / S0[:, None, None] - mu[:, :, None] * mu[:, None, :] + np.diag(phi)[None]
    return S0 / N, mu, Sigma


def gmm_estep_parameters(w, mu, Sigma):
    """(W [M, D, D] = L^-1 lower triangular, k [M]); LinAlgError naming the component whose Cholesky breaks down."""
    M, D = mu.shape
    W, k = np.empty_like(Sigma), np.empty(M)
    for m in range(M):
        try:
            L = np.linalg.cholesky(Sigma[m])
        except np.linalg.LinAlgError:
            raise np.linalg.LinAlgError("the covariance of component %d is not positive definite" % m) from None
        W[m] = np.tril(np.linalg.solve(L, np.eye(D)))
        k[m] = math.log(w[m]) - 0.5 * (D * math.log(2.0 * math.pi) + 2.0 * float(np.log(np.diag(L)).sum()))
    if not (np.all(np.isfinite(W)) and np.all(np.isfinite(k))):
        raise np.linalg.LinAlgError("the covariance of a component is numerically singular")
    return W, k


# ---- device work
class _Mixture:
    """The rows of one fit on the device, centred, and the buffers of its E and M steps."""

    def __init__(self, Z, zbar, M, device_index):
        self.torch, self.c, self.dev = _device(device_index)
        t = self.torch
        self.N, self.D, self.M = Z.shape[0], Z.shape[1], M
        self.Z = t.as_tensor(Z, device=self.dev) - t.as_tensor(zbar, device=self.dev)
        self.gamma = t.empty((self.N, M), dtype=t.float64, device=self.dev)
        self.ll = t.empty(self.N, dtype=t.float64, device=self.dev)

    def estep(self, mu, W, k):
        """(gamma on the device, ll float64[N] on the host)."""
        t = self.torch
        mu_d, W_d, k_d = (t.as_tensor(np.ascontiguousarray(a), device=self.dev) for a in (mu, W, k))
        self.c.gmm_estep(self.Z, self.N, self.D, self.M, mu_d, W_d, k_d, self.gamma, self.ll)
        return self.gamma, self.ll.cpu().numpy()

    def mstep(self, gamma):
        """(S0, S1, S2) on the host from responsibilities on the device."""
        t = self.torch
        words = self.c.gmm_work_len(self.N, self.D, self.M)
        _agree("the size of the M-step's work buffer", words, gmm_work_len(self.N, self.D, self.M))
        if getattr(self, "work", None) is None:
            self.work = t.empty(words, dtype=t.float64, device=self.dev)
            self.S0 = t.empty(self.M, dtype=t.float64, device=self.dev)
            self.S1 = t.empty((self.M, self.D), dtype=t.float64, device=self.dev)
            self.S2 = t.empty((self.M, self.D, self.D), dtype=t.float64, device=self.dev)
        self.c.gmm_mstep(self.Z, gamma, self.N, self.D, self.M, self.work, self.S0, self.S1, self.S2)
        return self.S0.cpu().numpy(), self.S1.cpu().numpy(), self.S2.cpu().numpy()


class _Codebook:
    """Rows on the device, float64 [N, ldz] of which the first D columns count, and the buffers of the two k-means steps
    for up to k centres; `labels` int32[N] on the device, all 0 at first."""

    def __init__(self, torch, c, dev, Z, D, k):
        self.torch, self.c, self.dev, self.Z, self.D = torch, c, dev, Z, D
        self.N, self.ldz = Z.shape
        words = c.kmeans_work_len(self.N, D, k)
        _agree("the size of the k-means update's work buffer", words, kmeans_work_len(self.N, D, k))
        self.words, self.k, self.work = words, k, None                  # the update's buffers come with the first update
        self.labels = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self.changed = torch.empty(-(-self.N // 64), dtype=torch.int32, device=dev)

    def assign(self, C):
        """labels <- the nearest of the centres C float64[K, D]; the number of rows whose label moved."""
        t = self.torch
        C = np.ascontiguousarray(C, dtype=np.float64)
        g = (C * C).sum(axis=1)
        self.c.kmeans_assign(self.Z, self.N, self.ldz, self.D, t.as_tensor(C, device=self.dev),
                             t.as_tensor(g, device=self.dev), len(C), self.labels, self.changed)
        return int(self.changed.sum().item())

    def update(self, K):
        """(count int64[K], S1[K, D], Q[K, D]) of the current labels, on the host."""
        if self.work is None:
            t, f64 = self.torch, self.torch.float64
            self.work = t.empty(self.words, dtype=f64, device=self.dev)
            self.count = t.empty(self.k, dtype=t.int64, device=self.dev)
            self.S1 = t.empty((self.k, self.D), dtype=f64, device=self.dev)
            self.Q = t.empty((self.k, self.D), dtype=f64, device=self.dev)
        self.c.kmeans_update(self.Z, self.N, self.ldz, self.D, self.labels, K, self.work, self.count, self.S1, self.Q)
        return self.count[:K].cpu().numpy(), self.S1[:K].cpu().numpy(), self.Q[:K].cpu().numpy()


def kmeans_grow(book, k, iters, split_iters):
    """The loop of DESIGN.md §12.3 on a _Codebook whose labels are all 0: (centres[k, D], counts, sse, rounds); the
    labels stay in `book`.  Only K x D sums and a count of moved rows come back from the device."""
    def lloyd(C):
        C = kmeans_moments(C, *book.update(len(C)))[0]
        return C, book.assign(C)
    C, rounds = np.zeros((1, book.D)), 0
    while len(C) < k:
        count, S1, Q = book.update(len(C))
        C, v, sse = kmeans_moments(C, count, S1, Q)
        C = kmeans_split(C, count, v, sse, k)
        book.assign(C)
        for _ in range(split_iters):
            C, _ = lloyd(C)
            rounds += 1
    for _ in range(iters):
        C, changed = lloyd(C)
        rounds += 1
        if changed == 0:
            break
    count, S1, Q = book.update(k)
    C, _, sse = kmeans_moments(C, count, S1, Q)
    return C, count, sse, rounds


def kmeans(Z, k, *, iters=20, split_iters=2, split=None, scale=None, device_index=0):
    """A codebook of `k` centres in [1, 64] for the rows of `Z` float64[N, D] (all finite, D <= 128, N >= 2 k), grown by
    splitting (Linde, Buzo & Gray 1980): from one centre, the clusters of largest squared error are split
    along their column of largest variance until there are k, `split_iters` Lloyd rounds after every growth and up to
    `iters` at k, stopping after a round in which no row moved.  Only the first `split` columns count when given.  The
    distance is Euclidean on the centred rows (on cepstral rows a log-spectral distance); scale="std" divides every
    column by its standard deviation first.  No random numbers: the same rows give the same codebook.  Returns
    dict(labels int64[N], centres float64[k, D'] in Z's coordinates, counts int64[k], sse float64[k] (each cluster's
    squared error about its centre, in the scaled coordinates when scale is given), rounds: the Lloyd rounds run).  Raises
    numpy.linalg.LinAlgError when the rows have fewer than k distinct clusters to split."""
    Z, k, iters, split_iters, split, scale = check_kmeans_arguments(Z, k, iters, split_iters, split, scale)
    rows, zbar, sd = kmeans_rows(Z, split, scale)
    torch, c, dev = _device(device_index)
    book = _Codebook(torch, c, dev, torch.as_tensor(rows, device=dev), rows.shape[1], k)
    C, count, sse, rounds = kmeans_grow(book, k, iters, split_iters)
    return dict(labels=book.labels.cpu().numpy().astype(np.int64), centres=C * sd + zbar, counts=count, sse=sse,
                rounds=rounds)


def kmeans_assign(centres, Z, *, device_index=0):
    """The label of each row of `Z` float64[N, D'] against a codebook `centres` float64[K, D'] (kmeans' centres, K <= 64,
    D' <= 128): the index of the nearest centre in the Euclidean distance, the lowest on a tie; int64[N].  Both are
    shifted by the mean of the centres before the scores are formed.  The distance is the plain Euclidean one: for a
    codebook grown with scale="std" on rows Z0 divide the rows and the centres by the numbers kmeans divided by,
    sd = Z0[:, :split].std(axis=0) with 1 in place of a 0, first: kmeans_assign(centres / sd, Z / sd)."""
    C = _rows(centres, "centres", GMM_MAX_COLUMNS)
    if len(C) > KMEANS_MAX_CENTRES:
        raise ValueError("centres must have 1 to %d rows, got %d" % (KMEANS_MAX_CENTRES, len(C)))
    Z = _rows(Z, "Z", GMM_MAX_COLUMNS)
    if Z.shape[1] != C.shape[1]:
        raise ValueError("Z must have the centres' %d columns, got %d" % (C.shape[1], Z.shape[1]))
    cbar = C.mean(axis=0)
    torch, c, dev = _device(device_index)
    book = _Codebook(torch, c, dev, torch.as_tensor(Z - cbar, device=dev), Z.shape[1], len(C))
    book.assign(C - cbar)
    return book.labels.cpu().numpy().astype(np.int64)


def _kmeans_responsibilities(mix, split):
    """The one-hot responsibilities of init="kmeans", written on the device: the labels of kmeans_grow on the mixture's
    own rows, their first `split` columns when given.  LinAlgError naming a final cluster without a row."""
    book = _Codebook(mix.torch, mix.c, mix.dev, mix.Z, split or mix.D, mix.M)
    _, count, _, _ = kmeans_grow(book, mix.M, **KMEANS_START)
    if np.any(count == 0):
        raise np.linalg.LinAlgError("the k-means start leaves component %d without a row"
                                    % int(np.flatnonzero(count == 0)[0]))
    return mix.gamma.zero_().scatter_(1, book.labels.long()[:, None], 1.0)


def gmm_fit(Z, components, *, iters=20, tol=1e-5, floor=1e-6, init=None, split=None, device_index=0):
    """Fits a Gaussian mixture with full covariances to the rows of `Z` float64[N, D] (all finite, D <= 128) by EM
    (DESIGN.md §12): `components` = M in [1, 64], N >= 2 M.  E and M steps alternate for at most `iters` rounds and stop
    after an E-step whose mean log-likelihood per row rose by less than `tol`.  `floor` x the variance of each column
    is added to the diagonal of every covariance.  `init` is an int array [N] of labels in [0, M), every label present;
    None sorts the rows along the principal axis of the standardised columns (the first `split` of them, all by default)
    and cuts them into M equal runs; "kmeans" takes the labels of a k-means codebook of M centres on the same columns
    (kmeans with its defaults; LinAlgError naming a centre that ends without a row).  Returns
    dict(weights[M], means[M, D], covs[M, D, D], zbar[D], phi[D], loglik[n_E_steps], n).  Raises numpy.linalg.LinAlgError naming the component when one is starved (its
    responsibilities sum to less than 1) or its covariance is not positive definite."""
    Z, M, iters, tol, floor, init, split = check_gmm_arguments(Z, components, iters, tol, floor, init, split)
    N, D = Z.shape
    zbar, phi = gmm_centre(Z, floor)
    mix = _Mixture(Z, zbar, M, device_index)
    if isinstance(init, str):
        first = _kmeans_responsibilities(mix, split)
    else:
        labels = gmm_init_labels(Z[:, :split] if split else Z, M) if init is None else init
        onehot = np.zeros((N, M))
        onehot[np.arange(N), labels] = 1.0
        first = mix.torch.as_tensor(onehot, device=mix.dev)
    w, mu, Sigma = gmm_finish_mstep(*mix.mstep(first), N, phi)
    loglik = []
    for _ in range(iters):
        gamma, ll = mix.estep(mu, *gmm_estep_parameters(w, mu, Sigma))
        loglik.append(math.fsum(ll) / N)
        if len(loglik) > 1 and loglik[-1] - loglik[-2] < tol:
            break
        w, mu, Sigma = gmm_finish_mstep(*mix.mstep(gamma), N, phi)
    return dict(weights=w, means=mu + zbar, covs=Sigma, zbar=zbar, phi=phi, loglik=np.array(loglik), n=N)


def gmm_posteriors(gmm, Z, *, device_index=0):
    """The E-step of a fitted mixture on rows `Z` float64[N, D]: (gamma float64[N, M], ll float64[N]), the
    responsibilities and the log-likelihood of each row."""
    w, mu, Sigma, zbar = check_gmm(gmm)
    Z = _rows(Z, "Z", GMM_MAX_COLUMNS)
    if Z.shape[1] != mu.shape[1]:
        raise ValueError("Z must have the mixture's %d columns, got %d" % (mu.shape[1], Z.shape[1]))
    mu_c = mu - zbar
    W, k = gmm_estep_parameters(w, mu_c, Sigma)
    mix = _Mixture(Z, zbar, len(w), device_index)
    gamma, ll = mix.estep(mu_c, W, k)
    return gamma.cpu().numpy(), ll
