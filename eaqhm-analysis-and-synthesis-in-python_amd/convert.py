"""Spectral conversion learned from aligned cepstral rows: a joint-density Gaussian mixture (not in the reference).

    gmm_fit(Z, components, *, iters=20, tol=1e-5, floor=1e-6, init=None, split=None, device_index=0)
        -> dict(weights[M], means[M, D], covs[M, D, D], zbar[D], phi[D], loglik[n_E_steps], n)
    gmm_posteriors(gmm, Z, *, device_index=0) -> (gamma[N, M], ll[N])
    conversion_pairs(CA, CB, path, span=None) -> (X, Y): the rows a model_align path pairs, empty rows dropped; with a
        span the dynamic rows [c | delta c] of both sides
    conversion_train(X, Y, components=8, *, level=False, iters=20, tol=1e-5, floor=1e-6, init=None, span=None, gv=None,
                     device_index=0)
        -> flat dict of arrays (np.savez): the gmm fields + dx, dy, level, A[M, dy, dx], b[M, dy], Wx[M, dx, dx], kx[M];
        with a span also span and py[M, dy], and dx, dy count the delta columns; with gv also gv_mean, gv_prec[dy / 2]
    conversion_apply(conv, C, *, device_index=0) -> float64[n, dy_cols] in model_cepstrum's layout (a static map)
    dynamic_rows(C, span=2, *, device_index=0) -> float64[n, 2 (P + 1)]: [c | delta c] over the runs of non-empty rows
    conversion_trajectory(conv, C, *, gv=None, gv_weight=1.0, gv_iters=30, trace=False, device_index=0)
        -> float64[n, Q + 1]: the most likely trajectory under a dynamic map, with the global-variance term when the map
        or `gv` carries its statistics; with trace=True also the objective float64[gv_iters + 1, dys]
    conversion_trajectory_em(conv, C, *, em_iters=4, em_tol=0.0, em_trace=False, gv=None, gv_weight=1.0, gv_iters=30,
                             trace=False, device_index=0)
        -> the same after `em_iters` EM refinements of the mixture sequence (reached as eaqhm_amd.convert.
        conversion_trajectory_em); with em_trace=True also the mean log-likelihood float64[iterations + 1]
    global_variance(C, level=False) -> float64[cols]: the variance of each mapped static column over the non-empty rows
    gv_statistics(utterances, *, level=False, rel_std=None) -> dict(gv_mean[dys], gv_prec[dys]) for conversion_train(gv=)
    f0_statistics(f0, voiced) -> (mean, std) of ln f0 over the voiced instants
    pitch_conversion_contour(f0, voiced, src_stats, tgt_stats) -> pitch_scale contour float64[n]
    kmeans(Z, k, *, iters=20, split_iters=2, split=None, scale=None, device_index=0)
        -> dict(labels int64[N], centres[k, D'], counts int64[k], sse[k], rounds): a codebook grown by splitting (LBG)
    kmeans_assign(centres, Z, *, device_index=0) -> int64[N]: the nearest centre of each row
    check_gmm_arguments, check_conversion_arguments, check_conversion, check_gv_arguments, check_kmeans_arguments,
    check_em_arguments: validation, no device work

The definition is DESIGN.md §12: EM with full covariances on centred rows (Dempster, Laird & Rubin 1977), the
regression of Stylianou, Cappe & Moulines (1998) in Kain & Macon's joint-density form.  Everything that scales with the
number of rows runs in libeaqhm_hip.so (eaqhm_gmm_estep, eaqhm_gmm_mstep, eaqhm_gmm_regress); the per-component algebra
(M Cholesky factors of D x D, their inverses, A_m) is host NumPy.  There is no CPU path.

DESIGN.md §12.1 adds the trajectory conversion of Toda, Black & Tokuda (2007): the mixture is trained on rows extended
with their delta features (eaqhm_ceps_delta) and an utterance is converted to the trajectory that is most likely under
the static and the delta statistics together (Tokuda et al. 2000): one banded positive-definite system per voiced run and
cepstral dimension (eaqhm_mlpg_solve).  DESIGN.md §12.2 adds the same paper's global-variance term: from that trajectory,
sweeps up the likelihood joined with a Gaussian prior on each column's variance over the utterance (eaqhm_gv_ascend).
DESIGN.md §12.3 adds the vector-quantisation codebook of Linde, Buzo & Gray (1980): centres grown by splitting, each
size settled by Lloyd rounds (eaqhm_kmeans_assign, eaqhm_kmeans_update); init="kmeans" starts the mixture from its
labels, the split decisions run on the host from K x D sums.
DESIGN.md §12.4 adds the 2007 paper's EM refinement of the mixture sequence: the component posteriors are revised in the
light of the trajectory they produce (eaqhm_mlpg_estep) and the trajectory is solved again, a few times over.
"""
import math

import numpy as np

from .align import _path
from .args import SCALE_RANGE, _integer, _numeric_1d
from .cepstrum import CEPSTRUM_MAX_ORDER, _cepstrum_rows, check_cepstrum_warp
from .records import _device

GMM_MAX_COLUMNS = 128      # D = dx + dy at most: nine 16-wide tile rows of [c | 1] in the M-step's registers
GMM_MAX_SIDE = 64          # dx, dy at most
GMM_MAX_COMPONENTS = 64
GMM_FLOOR_RANGE = (1e-12, 1e-1)
GMM_MAX_ITERS = 1000
GMM_CHUNK_MIN = 512        # rows of an M-step chunk at least
GMM_CHUNKS_MAX = 128       # chunks at most
DELTA_SPAN_RANGE = (1, 8)  # span L of the delta window: tau = 1 .. L on each side
GV_CHUNK_MIN = 64          # rows of a reduction chunk of the global-variance ascent at least
GV_CHUNKS_MAX = 512        # chunks at most
GV_WEIGHT_RANGE = (1e-6, 1e6)
GV_MAX_ITERS = 10000
GV_REL_STD_MAX = 10.0
EM_MAX_ITERS = 100         # refinements of the mixture sequence at most
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


def gv_chunk_rows(n):
    """Rows per reduction chunk of the global-variance ascent (include/eaqhm_gv.h): max(64, 64 ceil(ceil(n / 512) / 64)),
    a function of n alone."""
    per = -(-int(n) // GV_CHUNKS_MAX)
    return max(GV_CHUNK_MIN, -(-per // GV_CHUNK_MIN) * GV_CHUNK_MIN)


def gv_work_len(n, dy, span):
    """Doubles of the ascent's `work`: the band and q, n (2 span + 2) dy; a word per row; a second trajectory, n dy; five
    sums per (chunk, column) and one per chunk; two words per column."""
    chunks = -(-int(n) // gv_chunk_rows(n))
    return n * (2 * span + 2) * dy + n + n * dy + chunks * (5 * dy + 1) + 2 * dy


def kmeans_work_len(N, D, K):
    """Doubles of the k-means update's `work` (include/eaqhm_kmeans.h): ceil(N / R) K (2 D + 1), R the M-step's chunk."""
    return -(-int(N) // gmm_chunk_rows(N)) * K * (2 * D + 1)


# ---- validation (no device work)
def _rows(Z, name, max_cols):
    A = np.asarray(Z)
    if A.dtype.kind not in "iuf" or A.ndim != 2 or A.shape[0] < 1:
        raise ValueError("%s must be a 2-D array of numbers, one row per observation" % name)
    if not 1 <= A.shape[1] <= max_cols:
        raise ValueError("%s must have 1 to %d columns, got %d" % (name, max_cols, A.shape[1]))
    A = np.ascontiguousarray(A, dtype=np.float64)
    if not np.all(np.isfinite(A)):
        raise ValueError("%s must be finite" % name)
    return A


def _real(x, name, lo, hi):
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number" % name) from None
    if not (lo <= v <= hi):                       # NaN fails both
        raise ValueError("%s must be in [%g, %g], got %r" % (name, lo, hi, x))
    return v


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


def check_span(span):
    """The span of the delta window as an int in [1, 8]."""
    span = _integer(span, "span")
    if not DELTA_SPAN_RANGE[0] <= span <= DELTA_SPAN_RANGE[1]:
        raise ValueError("span must be in [%d, %d], got %d" % (DELTA_SPAN_RANGE + (span,)))
    return span


def check_conversion_arguments(X, Y, components=8, level=False, iters=20, tol=1e-5, floor=1e-6, init=None, span=None):
    """Validates everything conversion_train gets (no device work): returns (X, Y, level) with X, Y float64 rows.  With
    level=False column 0 stays out of the map.  Rows are cepstral rows, order 1 to 63, 2 to 64 columns: what
    conversion_apply and envelope= accept; so level=False maps at most 63 columns a side and level=True 64.  With a span
    the rows are dynamic rows [c | delta c], an even number of columns, and the mapped columns with their deltas are at
    most 64 a side (the regression's limit) and 128 together (the mixture's)."""
    if span is not None:
        span = check_span(span)
    width = (CEPSTRUM_MAX_ORDER + 1) * (1 if span is None else 2)
    X, Y = _rows(X, "X", width), _rows(Y, "Y", width)
    if X.shape[0] != Y.shape[0]:
        raise ValueError("X and Y must pair row by row, got %d and %d rows" % (X.shape[0], Y.shape[0]))
    if not isinstance(level, (bool, np.bool_)):
        raise ValueError("level must be True or False")
    if span is not None:
        for A, name in ((X, "X"), (Y, "Y")):
            if A.shape[1] % 2 or A.shape[1] < 4:
                raise ValueError("%s must be dynamic rows [c | delta c]: an even number of columns, 4 to %d, got %d"
                                 % (name, width, A.shape[1]))
        dx, dy = (A.shape[1] - (0 if level else 2) for A in (X, Y))
        if dx > GMM_MAX_SIDE or dy > GMM_MAX_SIDE or dx + dy > GMM_MAX_COLUMNS:
            raise ValueError("a dynamic map takes at most %d mapped columns a side with their deltas and %d together, got "
                             "%d and %d" % (GMM_MAX_SIDE, GMM_MAX_COLUMNS, dx, dy))
    for A, name in ((X, "X"), (Y, "Y")):
        if A.shape[1] < 2:
            raise ValueError("%s must have 2 to %d columns (order 1 to %d), got %d"
                             % (name, CEPSTRUM_MAX_ORDER + 1, CEPSTRUM_MAX_ORDER, A.shape[1]))
    check_gmm_arguments(np.zeros((X.shape[0], 1)), components, iters, tol, floor, init, None)
    return X, Y, bool(level)


_CONVERSION_FIELDS = ("weights", "means", "covs", "zbar", "phi", "loglik", "n", "dx", "dy", "level", "A", "b", "Wx", "kx")


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


def check_conversion(conv):
    """Validates a conversion dict (conversion_train's, or one loaded with np.load(allow_pickle=False)): every field,
    shapes, finiteness, the mixture's rules (check_gmm).  Returns a dict of float64 / int arrays ready for use."""
    for name in _CONVERSION_FIELDS:
        _field(conv, name)
    dx, dy = (int(_field(conv, k, ())) for k in ("dx", "dy"))
    level = bool(_field(conv, "level", ()))
    if not (1 <= dx <= GMM_MAX_SIDE and 1 <= dy <= GMM_MAX_SIDE):
        raise ValueError("the conversion's dx and dy must be in [1, %d]" % GMM_MAX_SIDE)
    w, mu, S, zbar = check_gmm(conv)
    M = len(w)
    if mu.shape[1] != dx + dy:
        raise ValueError("the conversion's means must have dx + dy = %d columns, got %d" % (dx + dy, mu.shape[1]))
    out = dict(weights=w, means=mu, covs=S, zbar=zbar, dx=dx, dy=dy, level=level)
    for name, shape in (("A", (M, dy, dx)), ("b", (M, dy)), ("Wx", (M, dx, dx)), ("kx", (M,)), ("phi", (dx + dy,))):
        out[name] = np.ascontiguousarray(_field(conv, name, shape), dtype=np.float64)
    if np.any(np.einsum("mii->mi", out["Wx"]) <= 0) or np.any(np.triu(out["Wx"], 1) != 0):
        raise ValueError("the conversion's Wx must be lower triangular with a positive diagonal")
    out["loglik"] = _field(conv, "loglik").astype(np.float64).reshape(-1)
    out["n"] = int(_field(conv, "n", ()))
    if _has(conv, "span"):                        # a dynamic map
        span = _field(conv, "span", ())
        if span.dtype.kind not in "iu":
            raise ValueError("the conversion's span must be an integer")
        out["span"] = check_span(int(span))
        if dx % 2 or dy % 2:
            raise ValueError("a dynamic conversion's dx and dy count the delta columns: they must be even")
        out["py"] = np.ascontiguousarray(_field(conv, "py", (M, dy)), dtype=np.float64)
        if np.any(out["py"] <= 0):
            raise ValueError("the conversion's py must be positive")
    if _has(conv, "gv_mean") or _has(conv, "gv_prec"):    # the global-variance statistics
        if "span" not in out:
            raise ValueError("the conversion's gv_mean and gv_prec need a dynamic map (span)")
        out.update(_gv_fields(conv, dy // 2, "the conversion"))
    if _has(conv, "cep_warp"):    # the axis of the rows the map was learned on; without it the linear one
        a = _field(conv, "cep_warp", ())
        if a.dtype.kind not in "iuf":
            raise ValueError("the conversion's cep_warp must be a number")
        out["cep_warp"] = check_cepstrum_warp(float(a), "the conversion's cep_warp")
    return out


def _gv_fields(gv, dys, what):
    """dict(gv_mean, gv_prec) float64[dys] of a mapping that must hold both: finite and > 0."""
    out = {}
    for name in ("gv_mean", "gv_prec"):
        try:
            a = np.asarray(gv[name])
        except (KeyError, TypeError, IndexError):
            raise ValueError("%s lacks the field %r" % (what, name)) from None
        if a.dtype.kind not in "iuf" or a.shape != (dys,):
            raise ValueError("%s's %s must be %d numbers, one per mapped static column, got shape %s"
                             % (what, name, dys, a.shape))
        a = np.ascontiguousarray(a, dtype=np.float64)
        if not (np.all(np.isfinite(a)) and np.all(a > 0)):
            raise ValueError("%s's %s must be finite and > 0" % (what, name))
        out[name] = a
    return out


def check_gv_arguments(conv, gv=None, gv_weight=1.0, gv_iters=30, trace=False):
    """Validates the global-variance arguments of conversion_trajectory against a validated dynamic map (check_conversion's
    result; no device work): returns (stats, gv_weight, gv_iters, trace), stats dict(gv_mean, gv_prec) float64[dys] or
    None when the ascent does not run (gv=False, or gv=None with a map that has no statistics)."""
    if "span" not in conv:
        raise ValueError("the global-variance term needs a dynamic map (span)")
    if gv is None:
        stats = {k: conv[k] for k in ("gv_mean", "gv_prec")} if "gv_mean" in conv else None
    elif isinstance(gv, (bool, np.bool_)):
        if gv:
            raise ValueError("gv must be None (the map's statistics), False or a gv_statistics dict")
        stats = None
    else:
        stats = _gv_fields(gv, conv["dy"] // 2, "gv")
    gv_weight = _real(gv_weight, "gv_weight", *GV_WEIGHT_RANGE)
    gv_iters = _integer(gv_iters, "gv_iters")
    if not 0 <= gv_iters <= GV_MAX_ITERS:
        raise ValueError("gv_iters must be in [0, %d], got %d" % (GV_MAX_ITERS, gv_iters))
    if not isinstance(trace, (bool, np.bool_)):
        raise ValueError("trace must be True or False")
    if trace and stats is None:
        raise ValueError("trace=True needs the global-variance term: a map with gv_mean and gv_prec, or gv=")
    return stats, gv_weight, gv_iters, bool(trace)


def check_em_arguments(em_iters=4, em_tol=0.0, em_trace=False):
    """Validates the refinement arguments of conversion_trajectory_em (no device work): returns (em_iters, em_tol,
    em_trace), em_iters an int in [0, 100], em_tol a finite float >= 0, em_trace a bool."""
    em_iters = _integer(em_iters, "em_iters")
    if not 0 <= em_iters <= EM_MAX_ITERS:
        raise ValueError("em_iters must be in [0, %d], got %d" % (EM_MAX_ITERS, em_iters))
    if isinstance(em_tol, (bool, np.bool_)):
        raise ValueError("em_tol must be a number")
    em_tol = _real(em_tol, "em_tol", 0.0, np.inf)
    if not np.isfinite(em_tol):
        raise ValueError("em_tol must be finite")
    if not isinstance(em_trace, (bool, np.bool_)):
        raise ValueError("em_trace must be True or False")
    return em_iters, em_tol, bool(em_trace)


def _has(conv, name):
    try:
        conv[name]
    except (KeyError, TypeError, IndexError):
        return False
    return True


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


def gmm_conversion_parameters(w, mu_c, Sigma, dx):
    """(A [M, dy, dx], b [M, dy], Wx [M, dx, dx], kx [M]) on centred coordinates: A_m = Sigma_m^yx (Sigma_m^xx)^-1,
    b_m = mu_m^y - A_m mu_m^x, and the E-step parameters of the marginal mixture on x."""
    Wx, kx = gmm_estep_parameters(w, np.ascontiguousarray(mu_c[:, :dx]), np.ascontiguousarray(Sigma[:, :dx, :dx]))
    A = np.stack([Sigma[m, dx:, :dx] @ Wx[m].T @ Wx[m] for m in range(len(w))])
    b = mu_c[:, dx:] - np.einsum("mij,mj->mi", A, mu_c[:, :dx])
    return np.ascontiguousarray(A), np.ascontiguousarray(b), Wx, kx


def gmm_conditional_precisions(Sigma, A, dx):
    """py [M, dy] = 1 / diag(Sigma_m^yy - A_m Sigma_m^xy): the reciprocal diagonals of the conditional covariances of y
    given x; LinAlgError naming the component when one is not positive."""
    py = np.empty((len(A), A.shape[1]))
    for m in range(len(A)):
        v = np.diag(Sigma[m, dx:, dx:]) - np.einsum("ij,ji->i", A[m], Sigma[m, :dx, dx:])
        if not np.all(v > 0) or not np.all(np.isfinite(1.0 / v)):
            raise np.linalg.LinAlgError("the conditional covariance of component %d has a diagonal entry that is not "
                                        "positive" % m)
        py[m] = 1.0 / v
    return py


def delta_runs(full):
    """(start, length) int64 arrays of the runs: the maximal stretches of True in the bool array `full`."""
    f = np.concatenate(([False], np.asarray(full, dtype=bool), [False]))
    edges = np.flatnonzero(f[1:] != f[:-1])
    return edges[0::2].astype(np.int64), (edges[1::2] - edges[0::2]).astype(np.int64)


def _dynamic_columns(D, cols, skip):
    """The mapped columns of dynamic rows of `cols` static columns: both halves without their first `skip` columns."""
    return np.ascontiguousarray(np.hstack((D[:, skip:cols], D[:, cols + skip:])))


def global_variance(C, level=False):
    """The population variance of each mapped static column of cepstral rows `C` float64[n, P + 1] over their non-empty
    rows: float64[P], or float64[P + 1] with level=True.  Host NumPy.  ValueError without a non-empty
    row."""
    C = _cepstrum_rows(C, "C")
    if not isinstance(level, (bool, np.bool_)):
        raise ValueError("level must be True or False")
    full = ~np.isneginf(C[:, 0])
    if not full.any():
        raise ValueError("global_variance needs at least one non-empty row")
    return C[full, 0 if level else 1:].var(axis=0)


def gv_statistics(utterances, *, level=False, rel_std=None):
    """The target speaker's global-variance statistics for conversion_train(gv=) and conversion_trajectory(gv=)
    (DESIGN.md §12.2): dict(gv_mean[dys], gv_prec[dys]) from a sequence of cepstral-row arrays, all of one width.  With
    rel_std=None gv_mean is the mean and gv_prec the reciprocal of the population variance of global_variance over at least
    2 utterances (ValueError when a variance is 0).  With `rel_std` in (0, 10] the spread is stated instead of measured:
    gv_prec = 1 / (rel_std gv_mean)^2, and one utterance suffices.  gv_mean must come out > 0 and finite."""
    try:
        rows = list(utterances)
    except TypeError:
        raise ValueError("utterances must be a sequence of cepstral-row arrays") from None
    if rel_std is not None:
        rel_std = _real(rel_std, "rel_std", 0.0, GV_REL_STD_MAX)
        if rel_std == 0.0:
            raise ValueError("rel_std must be in (0, %g]" % GV_REL_STD_MAX)
    if len(rows) < (2 if rel_std is None else 1):
        raise ValueError("gv_statistics needs at least %s" % ("2 utterances, or rel_std" if rel_std is None
                                                              else "1 utterance"))
    V = [global_variance(C, level) for C in rows]
    if any(v.shape != V[0].shape for v in V):
        raise ValueError("the utterances must all have the same number of columns")
    V = np.stack(V)
    mean = V.mean(axis=0)
    if not (np.all(np.isfinite(mean)) and np.all(mean > 0)):
        raise ValueError("a column's global variance is 0 or not finite: gv_mean must be > 0")
    if rel_std is None:
        var = V.var(axis=0)
        if np.any(var == 0):
            raise ValueError("a column's global variance is the same in every utterance: pass rel_std")
        prec = 1.0 / var
    else:
        prec = 1.0 / (rel_std * mean) ** 2
    if not np.all(np.isfinite(prec)):
        raise ValueError("gv_prec is not finite")
    return dict(gv_mean=mean, gv_prec=prec)


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
        if words != gmm_work_len(self.N, self.D, self.M):
            raise RuntimeError("libeaqhm_hip.so and the host disagree on the size of the M-step's work buffer")
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
        if words != kmeans_work_len(self.N, D, k):
            raise RuntimeError("libeaqhm_hip.so and the host disagree on the size of the k-means update's work buffer")
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


def conversion_pairs(CA, CB, path, span=None, *, device_index=0):
    """The rows a model_align path pairs: (X, Y) = (CA[i], CB[j]) for the pairs (i, j) of `path` int[L, 2], without the
    pairs in which either row is empty, (-inf, 0, .., 0).  np.vstack the results of several utterance pairs for
    conversion_train.  CA and CB may have different orders.  span=None is host only; with a `span` in [1, 8] the rows
    paired are the dynamic rows [c | delta c] of both sides (dynamic_rows: the deltas are taken on each utterance,
    before the pairing), for conversion_train(span=)."""
    CA, CB = _cepstrum_rows(CA, "CA"), _cepstrum_rows(CB, "CB")
    p, _ = _path(path, len(CA))
    if p[:, 1].max() >= len(CB):
        raise ValueError("path must pair instants of A with instants 0..%d of B" % (len(CB) - 1))
    if span is not None:
        span = check_span(span)
        CA, CB = (dynamic_rows(C, span, device_index=device_index) for C in (CA, CB))
    X, Y = CA[p[:, 0]], CB[p[:, 1]]
    keep = ~(np.isneginf(X[:, 0]) | np.isneginf(Y[:, 0]))
    return X[keep], Y[keep]


def dynamic_rows(C, span=2, *, device_index=0):
    """Cepstral rows `C` float64[n, P + 1] extended with their delta features: float64[n, 2 (P + 1)],
    row t = [c_t | delta c_t], delta c_t = sum_tau w_tau (c_clip(t + tau) - c_clip(t - tau)), tau = 1 .. span, w_tau =
    tau / (2 sum_k k^2).  `clip` holds the index inside the row's own run of consecutive non-empty rows (the edge row is
    repeated, the HTK convention), so nothing crosses an unvoiced gap and a run of one row has delta 0.  An empty row
    (-inf, 0, .., 0) gives (-inf, 0, .. | 0, ..).  `span` is in [1, 8]."""
    C = _cepstrum_rows(C, "C")
    span = check_span(span)
    torch, c, dev = _device(device_index)
    n, cols = C.shape
    out = torch.empty((n, cols), dtype=torch.float64, device=dev)
    c.ceps_delta(torch.as_tensor(C, device=dev), n, cols, span, out)
    return np.hstack((C, out.cpu().numpy()))


def conversion_train(X, Y, components=8, *, level=False, iters=20, tol=1e-5, floor=1e-6, init=None, span=None,
                     gv=None, device_index=0):
    """Learns the map from rows `X` float64[N, P + 1] to rows `Y` float64[N, Q + 1] (conversion_pairs') as a joint
    mixture of `components` Gaussians over [x | y].  level=False leaves column 0, the level c_0, out of
    both sides: conversion_apply copies it from the source row (a recording level is not a property of the speaker);
    level=True maps it like any other column.  The default initialisation and init="kmeans" (gmm_fit) look at the x
    columns only.  Returns a flat dict of arrays that np.savez stores and np.load(allow_pickle=False) returns: gmm_fit's fields, dx, dy, level,
    A[M, dy, dx], b[M, dy] and the marginal mixture's Wx[M, dx, dx], kx[M].
    With `span` in [1, 8] the rows are dynamic rows [c | delta c] (conversion_pairs(span=)) and the map is a dynamic one
    for conversion_trajectory: the mixture is over [x | delta x | y | delta y], level=False leaves
    column 0 and its delta out, dx and dy count the delta columns (at most 64 a side), and the dict gains span and
    py[M, dy], the reciprocal diagonals of the conditional covariances.  `gv`, a gv_statistics dict of the target speaker
    (span= only), is stored in the map as gv_mean[dy / 2] and gv_prec[dy / 2]: conversion_trajectory then adds the
    global-variance term."""
    X, Y, level = check_conversion_arguments(X, Y, components, level, iters, tol, floor, init, span)
    skip = 0 if level else 1
    if gv is not None:
        if span is None:
            raise ValueError("gv needs span=: a static map has no trajectory to trade against")
        gv = _gv_fields(gv, Y.shape[1] // 2 - skip, "gv")
    if span is None:
        x, y = X[:, skip:], Y[:, skip:]
    else:
        x, y = _dynamic_columns(X, X.shape[1] // 2, skip), _dynamic_columns(Y, Y.shape[1] // 2, skip)
    Z = np.ascontiguousarray(np.hstack((x, y)))
    dx, dy = x.shape[1], y.shape[1]
    g = gmm_fit(Z, components, iters=iters, tol=tol, floor=floor, init=init, split=dx, device_index=device_index)
    A, b, Wx, kx = gmm_conversion_parameters(g["weights"], g["means"] - g["zbar"], g["covs"], dx)
    g.update(n=np.int64(g["n"]), dx=np.int64(dx), dy=np.int64(dy), level=np.bool_(level), A=A, b=b, Wx=Wx, kx=kx)
    if span is not None:
        g.update(span=np.int64(check_span(span)), py=gmm_conditional_precisions(g["covs"], A, dx))
    if gv is not None:
        g.update(gv)
    return g


def conversion_apply(conv, C, *, device_index=0):
    """Converts cepstral rows `C` float64[n, dx_cols] (model_cepstrum's layout) with a conversion_train map: yhat_n =
    sum_m p(m | x_n) (b_m + A_m x_n).  An empty row (-inf, 0, .., 0) comes back empty; with level=False column 0 is the
    source row's.  Returns float64[n, dy_cols], accepted by eaQHMSynthesis(envelope=), model_from_parameters and
    cepstrum_envelope as it stands."""
    v = check_conversion(conv)
    if "span" in v:
        raise ValueError("this conversion is a dynamic map (span %d): use conversion_trajectory" % v["span"])
    skip = 0 if v["level"] else 1
    dx, dy, M = v["dx"], v["dy"], len(v["weights"])
    C = _cepstrum_rows(C, "C")
    if C.shape[1] != dx + skip:
        raise ValueError("C must have %d columns for this conversion, got %d" % (dx + skip, C.shape[1]))
    full = ~np.isneginf(C[:, 0])
    out = np.zeros((len(C), dy + skip))
    out[~full, 0] = -np.inf
    n = int(np.count_nonzero(full))
    if n == 0:
        return out
    mu_c = v["means"] - v["zbar"]
    mix = _Mixture(np.ascontiguousarray(C[full, skip:]), v["zbar"][:dx], M, device_index)
    gamma, _ = mix.estep(mu_c[:, :dx], v["Wx"], v["kx"])
    t = mix.torch
    Y = t.empty((n, dy), dtype=t.float64, device=mix.dev)
    mix.c.gmm_regress(mix.Z, gamma, t.as_tensor(v["A"], device=mix.dev), t.as_tensor(v["b"], device=mix.dev), n, dx, dy,
                      M, Y)
    out[full, skip:] = Y.cpu().numpy() + v["zbar"][dx:]
    if skip:
        out[full, 0] = C[full, 0]
    return out


def conversion_trajectory(conv, C, *, gv=None, gv_weight=1.0, gv_iters=30, trace=False, device_index=0):
    """Converts cepstral rows `C` float64[n, dx_cols] (model_cepstrum's layout) with a dynamic map, conversion_train(span=)'s,
    to the trajectory that is most likely under the static and the delta statistics together (Toda,
    Black & Tokuda 2007, the posterior-weighted initial estimate).  With X_t = [x_t | delta x_t], gamma the posteriors of
    the marginal mixture on X, P_t = sum_m gamma_tm py_m and r_t = sum_m gamma_tm py_m (b_m + A_m X_t) (un-centred), every
    run of non-empty rows and every static column d solves (diag(P^s) + W^T diag(P^D) W) y = r^s + W^T r^D, W the run's
    delta matrix.  Nothing couples across an empty row; an empty row comes back empty; with level=False column 0 is the
    source row's.  Returns float64[n, dy_cols], accepted wherever conversion_apply's result is.
    The global-variance term follows when there are statistics for it: gv=None takes the map's gv_mean
    and gv_prec if it has them, gv=False never does, a gv_statistics dict overrides the map.  From the trajectory above,
    scaled per column to the variance gv_mean, `gv_iters` sweeps (0 to 10000; 0 returns the scaled start) climb the
    likelihood joined with the prior of precision `gv_weight` gv_prec (gv_weight in [1e-6, 1e6]) on each column's
    variance over all non-empty rows.  A column that is constant, or an utterance of one non-empty row, stays as it is.
    trace=True returns (rows, float64[gv_iters + 1, dys]), the objective of every column before each sweep and after the
    last."""
    v = check_conversion(conv)
    if "span" not in v:
        raise ValueError("this conversion is a static map (no span): use conversion_apply")
    stats, gv_weight, gv_iters, trace = check_gv_arguments(v, gv, gv_weight, gv_iters, trace)
    out, objective, _ = _trajectory(v, C, stats, gv_weight, gv_iters, trace, device_index)
    return (out, objective) if trace else out


def conversion_trajectory_em(conv, C, *, em_iters=4, em_tol=0.0, em_trace=False, gv=None, gv_weight=1.0, gv_iters=30,
                             trace=False, device_index=0):
    """conversion_trajectory followed by the EM refinement of the mixture sequence (Toda, Black & Tokuda
    2007): conversion_trajectory's estimate y^(0) takes the component posteriors from the source rows alone, pi_tm =
    p(m | X_t).  Under the model the map implies, p(Y_t | X_t) = sum_m pi_tm N(Y_t; b_m + A_m X_t, diag(1 / py_m)) with
    Y_t(y) = [y_t | (W y)_t], each of `em_iters` iterations (0 to 100) revises the posteriors in the light of the
    trajectory, gamma_tm proportional to pi_tm N(Y_t(y^(i)); ..) (eaqhm_mlpg_estep), and solves conversion_trajectory's
    systems again with P and r formed from them: the exact maximiser of EM's auxiliary function, so the log-likelihood
    sum_t ln p(Y_t(y) | X_t) does not fall.  em_iters=0 is conversion_trajectory's result bit for bit.  The default of 4 is
    a stated choice, not a tuned one: on the cases of DESIGN.md §12.4 the gain falls by about a factor of ten per
    iteration.  With em_tol=0 all iterations run and nothing is read back between them; with em_tol > 0 the mean of the
    rows' log-likelihoods is formed on the host after every E-step, and the loop stops, keeping the trajectory that E-step
    scored, once the mean rose by less than em_tol over the previous iteration's.  The global-variance term (gv,
    gv_weight, gv_iters, trace: conversion_trajectory's) then starts from the last P, r and y; the posteriors stay fixed
    during the ascent.  Empty rows, level=False and the layout of `C` are conversion_trajectory's.  em_trace=True also
    returns float64[k + 1], the mean log-likelihood of y^(0) .. y^(k), k the iterations done (one more E-step at the end;
    a single 0 without a non-empty row).  Returns rows, then the objective if trace, then the log-likelihoods if
    em_trace.  A static map is a ValueError naming conversion_apply."""
    v = check_conversion(conv)
    if "span" not in v:
        raise ValueError("this conversion is a static map (no span): use conversion_apply")
    stats, gv_weight, gv_iters, trace = check_gv_arguments(v, gv, gv_weight, gv_iters, trace)
    em_iters, em_tol, em_trace = check_em_arguments(em_iters, em_tol, em_trace)
    out, objective, loglik = _trajectory(v, C, stats, gv_weight, gv_iters, trace, device_index,
                                         dict(iters=em_iters, tol=em_tol, trace=em_trace))
    result = (out,) + ((objective,) if trace else ()) + ((loglik,) if em_trace else ())
    return result if len(result) > 1 else out


def _trajectory(v, C, stats, gv_weight, gv_iters, trace, device_index, em=None):
    """What conversion_trajectory and conversion_trajectory_em share, from a validated dynamic map `v` and validated
    arguments: (rows, the ascent's objective or None, the refinement's mean log-likelihoods or None).  `em` is None or
    dict(iters, tol, trace); with None or iters = 0 the device work is conversion_trajectory's, launch for launch."""
    skip = 0 if v["level"] else 1
    span, dx, dy, M = v["span"], v["dx"], v["dy"], len(v["weights"])
    dxs, dys = dx // 2, dy // 2
    C = _cepstrum_rows(C, "C")
    if C.shape[1] != dxs + skip:
        raise ValueError("C must have %d columns for this conversion, got %d" % (dxs + skip, C.shape[1]))
    full = ~np.isneginf(C[:, 0])
    out = np.zeros((len(C), dys + skip))
    out[~full, 0] = -np.inf
    n = int(np.count_nonzero(full))
    if n == 0:
        return out, np.zeros((gv_iters + 1, dys)) if trace else None, np.zeros(1) if em and em["trace"] else None
    D = dynamic_rows(C, span, device_index=device_index)
    mu_c = v["means"] - v["zbar"]
    mix = _Mixture(_dynamic_columns(D[full], C.shape[1], skip), v["zbar"][:dx], M, device_index)
    gamma, _ = mix.estep(mu_c[:, :dx], v["Wx"], v["kx"])
    t, dev = mix.torch, mix.dev
    py = v["py"]
    r = t.empty((n, dy), dtype=t.float64, device=dev)
    pyA = t.as_tensor(np.ascontiguousarray(py[:, :, None] * v["A"]), device=dev)
    pyb = t.as_tensor(np.ascontiguousarray(py * (v["b"] + v["zbar"][dx:])), device=dev)
    mix.c.gmm_regress(mix.Z, gamma, pyA, pyb, n, dx, dy, M, r)
    py_d = t.as_tensor(py, device=dev)
    P = gamma @ py_d
    _, length = delta_runs(full)                       # the runs on the compacted rows: back to back
    start = np.concatenate(([0], np.cumsum(length)[:-1])).astype(np.int64)
    words = mix.c.mlpg_work_len(n, dys, span)
    if words != n * (2 * span + 2) * dys:
        raise RuntimeError("libeaqhm_hip.so and the host disagree on the size of the trajectory solve's work buffer")
    Y = t.empty((n, dys), dtype=t.float64, device=dev)
    P, start_d, length_d = P.contiguous(), t.as_tensor(start, device=dev), t.as_tensor(length, device=dev)
    work = t.empty(words, dtype=t.float64, device=dev)
    mix.c.mlpg_solve(P, r, n, dys, span, start_d, length_d, len(start), work, Y)
    loglik = None
    if em and (em["iters"] or em["trace"]):            # X, pi = gamma, the scaled parameters, the runs and work stay put
        kc = 0.5 * np.log(py).sum(axis=1) - dys * math.log(2.0 * math.pi)
        A_d, bq_d, kc_d = (t.as_tensor(np.ascontiguousarray(a), device=dev) for a in (v["A"], v["b"] + v["zbar"][dx:], kc))
        refined = t.empty((n, M), dtype=t.float64, device=dev)
        ll = t.empty(n, dtype=t.float64, device=dev)
        score = em["trace"] or em["tol"] > 0           # the only read-back of the loop: n doubles per E-step
        means = []

        def estep():
            mix.c.mlpg_estep(mix.Z, gamma, A_d, bq_d, py_d, kc_d, Y, n, dx, dys, M, span, start_d, length_d, len(start),
                             refined, ll)
            if score:
                means.append(math.fsum(ll.cpu().numpy()) / n)
        stopped = False
        for _ in range(em["iters"]):
            estep()
            if em["tol"] > 0 and len(means) > 1 and means[-1] - means[-2] < em["tol"]:
                stopped = True                         # Y is the trajectory this E-step scored; P and r are the ones behind it
                break
            P = (refined @ py_d).contiguous()
            mix.c.gmm_regress(mix.Z, refined, pyA, pyb, n, dx, dy, M, r)
            mix.c.mlpg_solve(P, r, n, dys, span, start_d, length_d, len(start), work, Y)
        if em["trace"]:
            if not stopped:
                estep()                                # the last trajectory's score; P and r do not follow it
            loglik = np.array(means)
    objective = None
    if stats is not None:                              # P, r, the runs and y_ML stay where they are
        words = mix.c.gv_work_len(n, dys, span)
        if words != gv_work_len(n, dys, span) or mix.c.gv_chunk_rows(n) != gv_chunk_rows(n):
            raise RuntimeError("libeaqhm_hip.so and the host disagree on the size of the global-variance ascent's work buffer")
        if trace:
            objective = t.empty((gv_iters + 1, dys), dtype=t.float64, device=dev)
        mix.c.gv_ascend(P, r, n, dys, span, start_d, length_d, len(start), t.as_tensor(stats["gv_mean"], device=dev),
                        t.as_tensor(gv_weight * stats["gv_prec"], device=dev), gv_iters,
                        t.empty(words, dtype=t.float64, device=dev), Y, objective)
    out[full, skip:] = Y.cpu().numpy()
    if skip:
        out[full, 0] = C[full, 0]
    return out, objective.cpu().numpy() if trace else None, loglik


# ---- pitch (host only)
def _f0_track(f0, voiced):
    f = _numeric_1d(f0, "f0")
    vo = np.asarray(voiced)
    if vo.shape != f.shape or vo.dtype.kind not in "biu":
        raise ValueError("voiced must be one flag per entry of f0")
    vo = vo.astype(bool)
    if not (np.all(np.isfinite(f[vo])) and np.all(f[vo] > 0)):
        raise ValueError("f0 must be finite and > 0 at the voiced instants")
    return f, vo


def f0_statistics(f0, voiced):
    """(mean, std) of ln f0 over the voiced instants (population std); ValueError without a voiced instant."""
    f, vo = _f0_track(f0, voiced)
    if not vo.any():
        raise ValueError("f0_statistics needs at least one voiced instant")
    lf = np.log(f[vo])
    return float(lf.mean()), float(lf.std())


def _stats(s, name):
    try:
        m, d = (float(x) for x in s)
    except (TypeError, ValueError):
        raise ValueError("%s must be (mean, std) of ln f0" % name) from None
    if not (np.isfinite(m) and np.isfinite(d) and d >= 0):
        raise ValueError("%s must be finite with std >= 0" % name)
    return m, d


def pitch_conversion_contour(f0, voiced, src_stats, tgt_stats):
    """The log-Gaussian normalisation of pitch: ln f0' = mean_t + (std_t / std_s) (ln f0 - mean_s) at the voiced
    instants (std_s = 0: the ratio is 1).  Returns the pitch_scale contour f0' / f0, float64[n], clipped to SCALE_RANGE,
    1 at the unvoiced instants.  Host only."""
    f, vo = _f0_track(f0, voiced)
    (ms, ds), (mt, dt) = _stats(src_stats, "src_stats"), _stats(tgt_stats, "tgt_stats")
    ratio = dt / ds if ds > 0 else 1.0
    out = np.ones(len(f))
    lf = np.log(f[vo])
    with np.errstate(over="ignore"):
        out[vo] = np.clip(np.exp(mt + ratio * (lf - ms) - lf), *SCALE_RANGE)
    return out
