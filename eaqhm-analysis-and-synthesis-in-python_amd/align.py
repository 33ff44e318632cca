"""Time alignment of two models: banded DTW over their cepstral rows.  The cost table and the
recursion run in libeaqhm_hip.so (eaqhm_cepstrum_cost, eaqhm_dtw); there is no CPU path.

    model_align(CA, CB, band=None, c0_weight=0.0, empty_cost=4.0, *, device_index=0) -> (path int64[L, 2], cost)
    check_model_align_arguments(CA, CB, band=None, c0_weight=0.0, empty_cost=4.0)
    dtw(cost, band=None, *, device_index=0) -> (path int64[L, 2], total); check_dtw_arguments(cost, band=None)
    band_centres(nA, nB) -> int64[nA]; band_min_radius(nA, nB) -> int; dense_to_band(cost, r) -> float64[nA, 2 r + 1]
    alignment_index(path, nA) -> float64[nA]; warp_rows(X, idx) -> rows of X at fractional indices
    alignment_time_scale(path, nA, step_ratio=1.0) -> float64[nA]
"""
import numpy as np

from .args import SCALE_RANGE, _integer, _numeric_1d
from .cepstrum import _cepstrum_rows
from .records import _device


# ---- time alignment of two models
def band_centres(nA, nB):
    """c_i = (2 i (nB-1) + (nA-1)) // (2 (nA-1)), int64[nA]: the row of B on the scaled diagonal at row i of A (0 when
    nA = 1)."""
    i = np.arange(nA, dtype=np.int64)
    if nA == 1:
        return np.zeros(1, dtype=np.int64)
    return (2 * i * np.int64(nB - 1) + np.int64(nA - 1)) // np.int64(2 * (nA - 1))


def band_min_radius(nA, nB):
    """The smallest half-width that admits a path: nB - 1 when nA = 1, else ceil((nB - 1) / (nA - 1))."""
    return nB - 1 if nA == 1 else -((1 - nB) // (nA - 1))


def _band_radius(band, nA, nB):
    """band=None is the full table, r = max(nA, nB) - 1; an integer is r itself (never more than the full table)."""
    full = max(nA, nB) - 1
    if band is None:
        return full
    r = _integer(band, "band")
    if r < band_min_radius(nA, nB):
        raise ValueError("band=%d admits no path between %d and %d rows: it needs band >= %d"
                         % (r, nA, nB, band_min_radius(nA, nB)))
    return min(r, full)


def dense_to_band(cost, r):
    """A dense float64[nA, nB] table in band layout float64[nA, 2 r + 1]: cell (i, j) at [i, j - c_i + r], +inf where
    the band leaves the table."""
    cost = np.asarray(cost, dtype=np.float64)
    nA, nB = cost.shape
    j = band_centres(nA, nB)[:, None] - r + np.arange(2 * r + 1, dtype=np.int64)[None, :]
    inside = (j >= 0) & (j < nB)
    out = np.full(j.shape, np.inf)
    out[inside] = cost[np.nonzero(inside)[0], j[inside]]
    return out


def _run_dtw(torch, c, band_d, nA, nB, r):
    """eaqhm_dtw on a device band: (path int64[L, 2], total)."""
    dev = c.device
    ptr = torch.empty(band_d.shape, dtype=torch.uint8, device=dev)
    path = torch.empty((nA + nB - 1, 2), dtype=torch.int32, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    c.dtw(band_d, nA, nB, r, ptr, path, n, total)
    L = int(n.item())
    if L < 1:
        raise RuntimeError("the alignment's back-pointers do not lead back to the start")
    return path[:L].cpu().numpy().astype(np.int64), float(total.item())


def _fits_device(torch, dev, nA, r):
    """The working set of an alignment, the band of costs and its back-pointers, 9 bytes per cell."""
    need = 9 * nA * (2 * r + 1)
    free = torch.cuda.mem_get_info(dev)[0]
    if need > free:
        raise ValueError("the alignment needs %d bytes for %d x %d band cells and the device has %d free: pass a "
                         "narrower band=" % (need, nA, 2 * r + 1, free))


def _cost_weight(x, name):
    try:
        x = float(x)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number" % name) from None
    if not (np.isfinite(x) and x >= 0):
        raise ValueError("%s must be finite and >= 0, got %r" % (name, x))
    return x


def check_model_align_arguments(CA, CB, band=None, c0_weight=0.0, empty_cost=4.0):
    """Validates everything model_align gets (no device work): returns (CA, CB, r, c0_weight, empty_cost)."""
    CA, CB = _cepstrum_rows(CA, "CA"), _cepstrum_rows(CB, "CB")
    if CA.shape[1] != CB.shape[1]:
        raise ValueError("CA and CB must have the same order, got %d and %d" % (CA.shape[1] - 1, CB.shape[1] - 1))
    return (CA, CB, _band_radius(band, len(CA), len(CB)), _cost_weight(c0_weight, "c0_weight"),
            _cost_weight(empty_cost, "empty_cost"))


def model_align(CA, CB, band=None, c0_weight=0.0, empty_cost=4.0, *, device_index=0):
    """Aligns two cepstra in time by dynamic time warping.  `CA` float64[nA, P + 1] and `CB`
    float64[nB, P + 1] are model_cepstrum's rows (or any such rows) of the same order.  The cost of pairing row i of A
    with row j of B is d = c0_weight dC_0^2 + 2 sum_p dC_p^2, dC = CA[i] - CB[j]: at c0_weight = 1 the mean over
    frequency of the squared difference of the two log envelopes; the default 0 ignores the level.  Two empty rows
    (-inf, 0, .., 0) cost 0, an empty row against any other `empty_cost`.  `band` is the half-width, in rows of B,
    around the straight line from (0, 0) to (nA - 1, nB - 1) that the path may use; None is the whole table.  Returns
    (path, cost): int64[L, 2], the pairs (i, j) from (0, 0) to (nA - 1, nB - 1) in steps of (1, 1), (1, 0), (0, 1),
    with the smallest sum of d, and that sum.  On equal sums the diagonal step is preferred, then (1, 0).  Raises
    ValueError when `band` admits no path or the band does not fit the device's free memory."""
    CA, CB, r, c0_weight, empty_cost = check_model_align_arguments(CA, CB, band, c0_weight, empty_cost)
    nA, nB, P = len(CA), len(CB), CA.shape[1] - 1
    torch, c, dev = _device(device_index)
    _fits_device(torch, dev, nA, r)
    band_d = torch.empty((nA, 2 * r + 1), dtype=torch.float64, device=dev)
    c.cepstrum_cost(torch.as_tensor(CA, device=dev), nA, torch.as_tensor(CB, device=dev), nB, P, c0_weight, empty_cost,
                    r, band_d)
    return _run_dtw(torch, c, band_d, nA, nB, r)


def check_dtw_arguments(cost, band=None):
    """Validates dtw's arguments (no device work): returns (cost float64[nA, nB], r)."""
    D = np.asarray(cost)
    if D.dtype.kind not in "iuf" or D.ndim != 2 or D.shape[0] < 1 or D.shape[1] < 1:
        raise ValueError("cost must be a 2-D array of numbers, one row per row of A and one column per row of B")
    D = np.ascontiguousarray(D, dtype=np.float64)
    if not np.all(np.isfinite(D)) or np.any(D < 0):
        raise ValueError("cost must be finite and >= 0")
    return D, _band_radius(band, *D.shape)


def dtw(cost, band=None, *, device_index=0):
    """Dynamic time warping over the caller's own costs: `cost` float64[nA, nB], finite and >= 0 (for instance
    model_align's cost plus an f0 or voicing term).  `band`, the path and the tie rule are model_align's.  Returns
    (path int64[L, 2], total)."""
    D, r = check_dtw_arguments(cost, band)
    nA, nB = D.shape
    torch, c, dev = _device(device_index)
    _fits_device(torch, dev, nA, r)
    return _run_dtw(torch, c, torch.as_tensor(dense_to_band(D, r), device=dev), nA, nB, r)


def _path(path, nA):
    p = np.asarray(path)
    nA = _integer(nA, "nA")
    if p.dtype.kind not in "iu" or p.ndim != 2 or p.shape[1] != 2 or len(p) < 1:
        raise ValueError("path must be an integer array [L, 2] of pairs (i, j)")
    if nA < 1 or p[:, 0].min() < 0 or p[:, 0].max() >= nA or p[:, 1].min() < 0:
        raise ValueError("path must pair instants 0..%d of A with instants >= 0 of B" % (nA - 1))
    count = np.bincount(p[:, 0], minlength=nA)
    if np.any(count == 0):
        raise ValueError("path leaves instant %d of A unmatched" % int(np.flatnonzero(count == 0)[0]))
    return p, count


def alignment_index(path, nA):
    """For each instant of A the mean of the B indices the path pairs with it: float64[nA], fractional where an
    instant of A is held over several of B.  warp_rows reads B's rows there."""
    p, count = _path(path, nA)
    return np.bincount(p[:, 0], weights=p[:, 1].astype(np.float64), minlength=len(count)) / count


def warp_rows(X, idx):
    """The rows of `X` (1-D: its entries) read at the fractional row indices `idx` by linear interpolation between the
    two neighbouring rows; indices are held at the ends; an integer index returns the row bit for bit.  A 2-D `X` may
    hold empty cepstral rows (-inf, 0, .., 0): the nearer neighbour decides (the lower one at a fraction of exactly
    0.5): the result is the empty row when it is empty, and a copy of it when only the farther one is.  Returns
    float64[len(idx)] or float64[len(idx), X.shape[1]], e.g. warp_rows(CB, alignment_index(path, len(CA))): B's
    envelope at A's instants."""
    X = np.asarray(X)
    if X.dtype.kind not in "iuf" or X.ndim not in (1, 2) or len(X) < 1:
        raise ValueError("X must be a 1-D or 2-D array of numbers with at least one row")
    X = X.astype(np.float64)
    t = _numeric_1d(idx, "idx")
    if not np.all(np.isfinite(t)):
        raise ValueError("idx must be finite")
    t = np.clip(t, 0.0, len(X) - 1.0)
    lo = np.floor(t).astype(np.int64)
    hi = np.minimum(lo + 1, len(X) - 1)
    u = t - lo
    near = np.where(u > 0.5, hi, lo)
    w = u if X.ndim == 1 else u[:, None]
    with np.errstate(invalid="ignore"):
        out = (1.0 - w) * X[lo] + w * X[hi]
    whole = u == 0.0
    out[whole] = X[lo[whole]]
    if X.ndim == 2:
        empty = np.isneginf(X[:, 0])
        copy = ~whole & (empty[lo] | empty[hi])
        out[copy] = X[near[copy]]
    return out


def alignment_time_scale(path, nA, step_ratio=1.0):
    """A time_scale contour that gives A the local tempo of B: clip(step_ratio * d alignment_index / d instant, 0.25,
    4), float64[nA] (numpy.gradient).  `step_ratio` is B's analysis step over A's.  The clip to eaQHMSynthesis's
    range makes the total length approximate: where B holds or skips more than a factor 4 the contour saturates."""
    try:
        step_ratio = float(step_ratio)
    except (TypeError, ValueError):
        raise ValueError("step_ratio must be a number") from None
    if not (np.isfinite(step_ratio) and step_ratio > 0):
        raise ValueError("step_ratio must be finite and > 0")
    idx = alignment_index(path, nA)
    if len(idx) < 2:
        raise ValueError("a time-scale contour needs at least two instants of A")
    return np.clip(step_ratio * np.gradient(idx), *SCALE_RANGE)
