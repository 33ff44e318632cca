"""The argument rules that take no model: scales, contours, breakpoint curves, integers, reals in a range, rows of
numbers, seeds, frequency grids and formant-warp breakpoints.  Host only, NumPy only; every other module of the model layer validates through these.

    SCALE_RANGE = (0.25, 4.0): the range of every scale and of every segment slope of a formant warp
    FORMANT_WARP_MAX = 16: breakpoints of a formant warp at most
    check_curve(times_s, values, name="curve") -> (times, values) float64, validated

The underscore helpers are shared by records, cepstrum, align, noise, model, mixture, dynamics, mapping, convert,
nonparallel and cli: _scale, _sample_rate, _is_contour, _numeric_1d, _in_range, _contour, _integer, _real, _rows, _seed,
_freq_grid, _warp_rows, _warp_excludes_scale.
"""
import numpy as np

SCALE_RANGE = (0.25, 4.0)


def _scale(x, name):
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number" % name) from None
    if not np.isfinite(v) or not (SCALE_RANGE[0] <= v <= SCALE_RANGE[1]):
        raise ValueError("%s must be finite and in [%g, %g], got %r" % (name, SCALE_RANGE[0], SCALE_RANGE[1], x))
    return v


def _sample_rate(fs):
    try:
        fs = float(fs)
    except (TypeError, ValueError):
        raise ValueError("fs must be a number") from None
    if not np.isfinite(fs) or fs <= 0:
        raise ValueError("fs must be finite and > 0")
    return fs


def _is_contour(x):
    """True for an array-like scale (a contour); numbers and strings are scalars."""
    return not isinstance(x, (str, bytes)) and np.ndim(x) > 0


def _numeric_1d(x, name):
    a = np.asarray(x)
    if a.dtype.kind not in "iuf":
        raise ValueError("%s must hold numbers" % name)
    if a.ndim != 1:
        raise ValueError("%s must be 1-D, got shape %s" % (name, a.shape))
    return a.astype(np.float64)


def _in_range(v, name):
    if not np.all(np.isfinite(v)) or np.any(v < SCALE_RANGE[0]) or np.any(v > SCALE_RANGE[1]):
        raise ValueError("%s must be finite and in [%g, %g]" % (name, SCALE_RANGE[0], SCALE_RANGE[1]))
    return v


def _contour(x, name, n):
    """A scale as float64[n]: a number broadcast, or a 1-D array of n values."""
    if not _is_contour(x):
        return np.full(n, _scale(x, name))
    v = _numeric_1d(x, name)
    if len(v) != n:
        raise ValueError("%s must have one value per analysis instant (%d), got %d" % (name, n, len(v)))
    return _in_range(v, name)


def check_curve(times_s, values, name="curve"):
    """Validates a breakpoint curve (seconds, scale): returns (times, values) as float64 arrays.  The times must be
    finite and strictly increasing, the values finite and in SCALE_RANGE."""
    t = _numeric_1d(times_s, name + " times")
    v = _numeric_1d(values, name + " values")
    if len(t) == 0 or len(t) != len(v):
        raise ValueError("%s: times and values must be non-empty and of the same length" % name)
    if not np.all(np.isfinite(t)) or np.any(np.diff(t) <= 0):
        raise ValueError("%s: times must be finite and strictly increasing" % name)
    return t, _in_range(v, name + " values")


FORMANT_WARP_MAX = 16    # breakpoints of a formant warp at most: the kernels keep a row in 16 doubles of LDS per wave


def _warp_rows(formant_warp, rows, per):
    """A formant warp (f_in, f_out) as (float64[B], float64[rows, B]), validated: f_in is [B], f_out [B] or [rows, B]
    (one row per `per`), 1 <= B <= 16; all values finite and > 0; f_in and every row of f_out strictly increasing; every
    segment slope, the one from the origin included, in SCALE_RANGE."""
    try:
        f_in, f_out = formant_warp
    except (TypeError, ValueError):
        raise ValueError("formant_warp must be the pair (f_in, f_out) of breakpoint frequencies in Hz") from None
    x, y = np.asarray(f_in), np.asarray(f_out)
    if x.dtype.kind not in "iuf" or y.dtype.kind not in "iuf":
        raise ValueError("formant_warp must hold numbers")
    if x.ndim != 1:
        raise ValueError("formant_warp f_in must be 1-D, got shape %s" % (x.shape,))
    B = len(x)
    if not 1 <= B <= FORMANT_WARP_MAX:
        raise ValueError("formant_warp must have 1 to %d breakpoints, got %d" % (FORMANT_WARP_MAX, B))
    if y.shape != (B,) and y.shape != (rows, B):
        raise ValueError("formant_warp f_out must have shape (%d,) or one row per %s (%d, %d), got %s"
                         % (B, per, rows, B, y.shape))
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(np.broadcast_to(y, (rows, B)), dtype=np.float64)
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))) or np.any(x <= 0) or np.any(y <= 0):
        raise ValueError("formant_warp frequencies must be finite and > 0 (the map starts at (0, 0) by itself)")
    if np.any(np.diff(x) <= 0) or np.any(np.diff(y, axis=1) <= 0):
        raise ValueError("formant_warp f_in and every row of f_out must be strictly increasing")
    slope = np.diff(y, axis=1, prepend=0.0) / np.diff(x, prepend=0.0)
    if np.any(slope < SCALE_RANGE[0]) or np.any(slope > SCALE_RANGE[1]):
        raise ValueError("formant_warp: every segment slope (the one from the origin included) must be in [%g, %g]"
                         % SCALE_RANGE)
    return x, y


def _warp_excludes_scale(formant_scale):
    if _is_contour(formant_scale) or _scale(formant_scale, "formant_scale") != 1.0:
        raise ValueError("formant_warp and formant_scale exclude each other: B = 1 with (x, alpha x) is the scale alpha")


def _freq_grid(freqs):
    f = _numeric_1d(freqs, "freqs")
    if len(f) == 0 or len(f) > 2 ** 31 - 1 or not np.all(np.isfinite(f)) or np.any(f < 0):
        raise ValueError("freqs must be a non-empty 1-D array of finite frequencies >= 0 (Hz)")
    return f


def _integer(x, name):
    if isinstance(x, (bool, np.bool_)):
        raise ValueError("%s must be an integer" % name)
    try:
        ok = float(x).is_integer()
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("%s must be an integer, got %r" % (name, x))
    return int(x)


def _real(x, name, lo, hi):
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number" % name) from None
    if not (lo <= v <= hi):                       # NaN fails both
        raise ValueError("%s must be in [%g, %g], got %r" % (name, lo, hi, x))
    return v


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


def _seed(seed):
    seed = _integer(seed, "seed")
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2**64)")
    return seed
