"""Delta rows and global-variance statistics of cepstral rows (not in the reference): what a dynamic map is trained on
and what its trajectory is held to.  Nothing here knows of a map; the second layer below convert.

    dynamic_rows(C, span=2, *, device_index=0) -> float64[n, 2 (P + 1)]: [c | delta c] over the runs of non-empty rows
    check_span(span) -> int in DELTA_SPAN_RANGE
    delta_runs(full) -> (start, length): the runs of True
    _dynamic_columns(D, cols, skip): the mapped columns of dynamic rows
    global_variance(C, level=False) -> float64[cols]: the variance of each mapped static column over the non-empty rows
    gv_statistics(utterances, *, level=False, rel_std=None) -> dict(gv_mean[dys], gv_prec[dys])
    _gv_fields(gv, dys, what): the two fields of such a dict, validated
    mlpg_work_len, gv_chunk_rows, gv_work_len: host mirrors of the library's buffer sizes

The deltas are DESIGN.md §12.1 and run in libeaqhm_hip.so (eaqhm_ceps_delta); the statistics are DESIGN.md §12.2 and
host NumPy.  The size mirrors belong to eaqhm_mlpg_solve and eaqhm_gv_ascend, which convert drives.
"""
import numpy as np

from .args import _integer, _real
from .cepstrum import _cepstrum_rows
from .records import _device

DELTA_SPAN_RANGE = (1, 8)  # span L of the delta window: tau = 1 .. L on each side
GV_CHUNK_MIN = 64          # rows of a reduction chunk of the global-variance ascent at least
GV_CHUNKS_MAX = 512        # chunks at most
GV_REL_STD_MAX = 10.0


def check_span(span):
    """The span of the delta window as an int in [1, 8]."""
    span = _integer(span, "span")
    if not DELTA_SPAN_RANGE[0] <= span <= DELTA_SPAN_RANGE[1]:
        raise ValueError("span must be in [%d, %d], got %d" % (DELTA_SPAN_RANGE + (span,)))
    return span


def delta_runs(full):
    """(start, length) int64 arrays of the runs: the maximal stretches of True in the bool array `full`."""
    f = np.concatenate(([False], np.asarray(full, dtype=bool), [False]))
    edges = np.flatnonzero(f[1:] != f[:-1])
    return edges[0::2].astype(np.int64), (edges[1::2] - edges[0::2]).astype(np.int64)


def _dynamic_columns(D, cols, skip):
    """The mapped columns of dynamic rows of `cols` static columns: both halves without their first `skip` columns."""
    return np.ascontiguousarray(np.hstack((D[:, skip:cols], D[:, cols + skip:])))


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


# ---- global variance (host only)
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


# ---- host mirrors of the library's buffer sizes
def gv_chunk_rows(n):
    """Rows per reduction chunk of the global-variance ascent (include/eaqhm_gv.h): max(64, 64 ceil(ceil(n / 512) / 64)),
    a function of n alone."""
    per = -(-int(n) // GV_CHUNKS_MAX)
    return max(GV_CHUNK_MIN, -(-per // GV_CHUNK_MIN) * GV_CHUNK_MIN)


def mlpg_work_len(n, dy, span):
    """Doubles of the trajectory solve's `work` (include/eaqhm_mlpg.h): the band and q, n (2 span + 2) dy."""
    return n * (2 * span + 2) * dy


def gv_work_len(n, dy, span):
    """Doubles of the ascent's `work`: the band and q, n (2 span + 2) dy; a word per row; a second trajectory, n dy; five
    sums per (chunk, column) and one per chunk; two words per column."""
    chunks = -(-int(n) // gv_chunk_rows(n))
    return n * (2 * span + 2) * dy + n + n * dy + chunks * (5 * dy + 1) + 2 * dy
