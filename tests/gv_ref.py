"""TEST-ONLY NumPy model of DESIGN.md §12.2, the global-variance ascent from the maximum-likelihood trajectory, on the
dense R and q of tests/mlpg_ref.py (system), kept as their bands.  Runnable in float64 and np.longdouble.  `gv_term=False`
drops the global-variance term from g and h (the start stays the scaled one): what the result would be had the kernel
forgotten it."""
import numpy as np

import mlpg_ref as R

LD = np.longdouble


def bands(P, r, span, run_start, run_len, dtype=np.float64):
    """Per run (start, T, ab [2 span + 1, T, dy], q [T, dy]): ab[k, i] = R[i, i - k] of mlpg_ref.system, 0 where i < k."""
    dy = P.shape[1] // 2
    out = []
    for s, T in zip(run_start, run_len):
        s, T = int(s), int(T)
        ab = np.zeros((2 * span + 1, T, dy), dtype=dtype)
        q = np.zeros((T, dy), dtype=dtype)
        for d in range(dy):
            Rm, q[:, d] = R.system(P[s:s + T], r[s:s + T], span, d, dtype)
            assert not np.any(np.tril(Rm, -(2 * span + 1)))
            for k in range(min(2 * span, T - 1) + 1):
                ab[k, k:, d] = np.diagonal(Rm, -k)
        out.append((s, T, ab, q))
    return out


def apply_R(sys, y):
    """R y over all runs; y float[n, dy], rows outside the runs come back 0."""
    out = np.zeros_like(y)
    for s, T, ab, _ in sys:
        v, o = y[s:s + T], out[s:s + T]
        o += ab[0] * v
        for k in range(1, min(ab.shape[0], T)):
            o[k:] += ab[k, k:] * v[:-k]
            o[:-k] += ab[k, k:] * v[k:]
    return out


def ascend(sys, n, span, gv_mean, gv_prec, iters, y_ml, dtype=np.float64, gv_term=True):
    """(Y [n, dy], trace [iters + 1, dy], mag [iters + 1, dy]) from y_ml float64[n, dy] (NaN outside the runs, which stay
    NaN): the definition of §12.2 column by column, all columns at once.  mag is the sum of the magnitudes of the two
    terms of each trace entry.  gv_prec has the weight folded in."""
    live = np.zeros(n, dtype=bool)
    for s, T, _, _ in sys:
        live[s:s + T] = True
    N = int(live.sum())
    dy = y_ml.shape[1]
    mu, pv = np.asarray(gv_mean, dtype=np.float64).astype(dtype), np.asarray(gv_prec, dtype=np.float64).astype(dtype)
    q = np.zeros((n, dy), dtype=dtype)
    diag = np.zeros((n, dy), dtype=dtype)
    for s, T, ab, qq in sys:
        q[s:s + T], diag[s:s + T] = qq, ab[0]
    omega = dtype(1) / (2 * N)

    def moments(y):
        m = y[live].sum(axis=0) / N
        return m, ((y[live] - m) ** 2).sum(axis=0) / N

    def objective(y, Ry, v):
        a = -(omega / 2) * ((y[live] * Ry[live]).sum(axis=0) - 2 * (q[live] * y[live]).sum(axis=0))
        b = -(pv * (v - mu) ** 2) / 2
        return a + b, np.abs(a) + np.abs(b)

    y0 = np.where(live[:, None], y_ml, 0.0).astype(dtype)
    m, v = moments(y0)
    frozen = (v == 0) | (N < 2)
    L_ml, mag_ml = objective(y0, apply_R(sys, y0), v)
    scale = np.sqrt(mu / np.where(frozen, 1, v))
    y = np.where(frozen, y0, m + scale * (y0 - m))
    trace = np.zeros((iters + 1, dy), dtype=dtype)
    mag = np.zeros((iters + 1, dy), dtype=dtype)
    for k in range(iters + 1):
        m, v = moments(y)
        Ry = apply_R(sys, y)
        L, mg = objective(y, Ry, v)
        trace[k], mag[k] = np.where(frozen, L_ml, L), np.where(frozen, mag_ml, mg)
        if k == iters:
            break
        g = omega * (q - Ry)
        h = (4 * span + 1) * omega * diag
        if gv_term:
            g = g - pv * (v - mu) * (dtype(2) / N) * (y - m)
            h = h + pv * (dtype(2) / N) * (np.abs(v - mu) + 2 * v)
        y = np.where(frozen | ~live[:, None], y, y + g / np.where(live[:, None], h, 1))
    out = np.full((n, dy), np.nan, dtype=dtype)
    out[live] = np.where(frozen, y_ml[live].astype(dtype), y[live])
    return out, trace, mag


def variance(Y, live=None):
    """v of every column over the rows that are not NaN."""
    Y = np.asarray(Y)
    keep = ~np.isnan(Y[:, 0]) if live is None else live
    return Y[keep].var(axis=0)


# ---- the hand-built cases of tests/test_gpu_gv.py (seeded; the runs are (start, length) on n rows)
def back_to_back(lengths):
    length = np.array(lengths, dtype=np.int64)
    return np.concatenate(([0], np.cumsum(length)[:-1])).astype(np.int64), length, int(length.sum())


def spaced(lengths, gap=2):
    """The runs separated by `gap` rows that belong to no run, `gap` more in front and one behind."""
    length = np.array(lengths, dtype=np.int64)
    start = gap + np.concatenate(([0], np.cumsum(length + gap)[:-1]))
    return start.astype(np.int64), length, int(start[-1] + length[-1] + 1)


def inputs(n, dy, seed):
    """P, r float64[n, 2 dy]: P^s in [1/e, e], P^D / P^s from 0.1 to 100 row by row."""
    rng = np.random.default_rng(seed)
    P = np.exp(rng.uniform(-1.0, 1.0, (n, 2 * dy)))
    P[:, dy:] = P[:, :dy] * 10.0 ** rng.uniform(-1.0, 2.0, (n, 1))
    return P, rng.standard_normal((n, 2 * dy)) * P * 3.0


def statistics(y_ml, ratios, rel_stds):
    """gv_mean = ratio x v(y_ML) and gv_prec = 1 / (rel_std gv_mean)^2, the ratios and rel_stds dealt out over the columns in
    turn; a column of variance 0 gets gv_mean 1."""
    v = variance(y_ml)
    dy = len(v)
    mean = np.where(v > 0, v, 1.0) * np.resize(np.asarray(ratios, dtype=np.float64), dy)
    return mean, 1.0 / (np.resize(np.asarray(rel_stds, dtype=np.float64), dy) * mean) ** 2


CASES = {   # name: (span, runs, dys, iters, seed)
    "A": (1, back_to_back([200]), 1, 30, 1),
    "B": (2, back_to_back([1, 2, 3, 4, 5, 9, 700, 37]), 17, 30, 2),
    "C": (8, back_to_back([16, 17, 33, 300]), 64, 30, 3),
    "D1": (2, back_to_back([1]), 3, 5, 4),
    "D2": (2, back_to_back([2]), 3, 30, 5),
    "E": (2, spaced([1, 2, 3, 4, 5, 9, 700, 37]), 17, 30, 6),
    "F": (2, back_to_back([150]), 3, 30, 7),
    "G": (2, back_to_back([100, 65]), 2, 30, 8),       # 165 = 2 gv_chunk_rows(165) + 37
    "H": (2, back_to_back([40, 90]), 5, 0, 9),
}
RATIOS = (0.25, 0.5, 1.0, 2.0, 4.0, 0.7, 1.5)
REL_STDS = (0.15, 0.02)

_BUILT = {}


def case(name):
    """dict(span, start, length, n, dy, iters, P, r, y_ml, gv_mean, gv_prec, sys64, sysld, ref64 = (Y, trace, mag),
    refld, nogv = the float64 result without the term), built once."""
    if name in _BUILT:
        return _BUILT[name]
    span, (start, length, n), dy, iters, seed = CASES[name]
    P, r = inputs(n, dy, seed)
    y_ml = R.solve(P, r, span, start, length)
    if name == "F":                                     # a constant column: 0.75 k is exact for every k, so v = 0 exactly
        y_ml[:, 1] = 0.75
    mean, prec = statistics(y_ml, RATIOS, REL_STDS)
    c = dict(span=span, start=start, length=length, n=n, dy=dy, iters=iters, P=P, r=r, y_ml=y_ml, gv_mean=mean, gv_prec=prec)
    c["sys64"], c["sysld"] = bands(P, r, span, start, length), bands(P, r, span, start, length, LD)
    c["ref64"] = ascend(c["sys64"], n, span, mean, prec, iters, y_ml)
    c["refld"] = ascend(c["sysld"], n, span, mean, prec, iters, y_ml, LD)
    c["nogv"] = ascend(c["sys64"], n, span, mean, prec, iters, y_ml, gv_term=False)
    _BUILT[name] = c
    return c


U = 2.0 ** -53


def bars(c):
    """(bar on Y, bar on the trace [iters + 1, dy]) of a case: 100 x max(the float64 model's own difference from the
    long-double model, u max|Y|), and the same with u x the sum of the magnitudes of a trace entry's two terms."""
    (y64, t64, _), (yld, tld, mag) = c["ref64"], c["refld"]
    live = ~np.isnan(y64[:, 0])
    own = float(np.abs(y64[live].astype(LD) - yld[live]).max())
    bar_y = 100.0 * max(own, U * float(np.abs(yld[live]).max()))
    own_t = float(np.abs(t64.astype(LD) - tld).max())
    bar_t = 100.0 * np.maximum(own_t, U * mag.astype(np.float64))
    return bar_y, bar_t
