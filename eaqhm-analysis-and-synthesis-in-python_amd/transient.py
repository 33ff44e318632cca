"""Transient onsets and a time scale that leaves them alone: where a signal's bursts and sharp attacks
are, through libeaqhm_hip.so (eaqhm_onset_bands, eaqhm_onset_flux, eaqhm_onset_peaks), and the time-scale contour that
plays those places at their own duration and stretches the rest a little more.

    onset_strength(s, fs, *, hop=None, window=None, bands=24, fmin=100.0, lag=2, floor=1e-9, return_bands=False,
                   device_index=0) -> dict(d float64[Nf], hop, window, fs, length) (+ L float64[Nf, bands])
    onsets(od, *, delta=0.5, pre_max=3, post_max=3, pre_avg=20, post_avg=6, wait=10, device_index=0)
                   -> dict(frames int64[K], times float64[K] in seconds, strength float64[K])
    protection_weight(DetComponents, fs, times, *, before=0.010, after=0.040, ramp=0.010) -> p float64[No_ti], host only
    protect_time_scale(DetComponents, fs, length, time_scale, times, *, before=0.010, after=0.040, ramp=0.010,
                   return_info=False) -> rho' float64[No_ti] for eaQHMSynthesis(time_scale=), host only
    onset_plan(fs, window=None, bands=24, fmin=100.0) -> (win float64[w], k int32[bands + 1]), host only, no GPU needed
    keep_onsets(flagged, wait) -> the flagged frames the `wait` rule keeps, host only
    whole_frames(n, hop, window) -> (first, last) whole frame; first > last: none

Argument checks without device work: check_onset_arguments(s, fs, hop, window, bands, fmin, lag, floor),
check_strength(od), check_peak_arguments(delta, pre_max, post_max, pre_avg, post_avg, wait), check_onset_times(times),
check_protection_arguments(DetComponents, fs, times, before, after, ramp).  Constants: ONSET_WINDOW_RANGE, ONSET_HOP_MAX,
ONSET_BANDS_MAX, ONSET_LAG_MAX, ONSET_SPAN_MAX.

This module is reached as eaqhm_amd.transient; the package does not re-export it, and eaQHMSynthesis does not change:
the contour goes in as its time_scale, best with phase="shape", which keeps a burst's waveform at a local rate of 1, and
with noise=, which follows the same time map.  There is no CPU path: without the library or a GPU onset_strength and
onsets raise.
"""
import numpy as np

from .args import SCALE_RANGE, _contour, _integer, _numeric_1d, _sample_rate
from .swipe import erbs2hz, hz2erbs

ONSET_WINDOW_RANGE = (32, 2048)   # EAQHM_ONSET_WMIN, EAQHM_ONSET_WMAX
ONSET_HOP_MAX = 4096              # EAQHM_ONSET_HOP
ONSET_BANDS_MAX = 64              # EAQHM_ONSET_BANDS
ONSET_LAG_MAX = 16                # EAQHM_ONSET_LAG
ONSET_SPAN_MAX = 64               # EAQHM_ONSET_SPAN


def _number(v, name, lo=None, above=None):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (name, v)) from None
    if not np.isfinite(v) or (lo is not None and v < lo) or (above is not None and not v > above):
        raise ValueError("%s must be finite%s, got %r" % (name, " and >= %g" % lo if lo is not None else
                                                          " and > %g" % above if above is not None else "", v))
    return v


def _in(v, name, lo, hi):
    v = _integer(v, name)
    if not lo <= v <= hi:
        raise ValueError("%s must be in [%d, %d], got %d" % (name, lo, hi, v))
    return v


def _device_index(device_index):
    if isinstance(device_index, bool) or not isinstance(device_index, (int, np.integer)) or device_index < 0:
        raise ValueError("device_index must be a non-negative integer, got %r" % (device_index,))
    return int(device_index)


# ---- the plan
def _window_length(fs, window):
    if window is None:
        window = ONSET_WINDOW_RANGE[0]
        while window < 0.010 * fs and window < 2 * ONSET_WINDOW_RANGE[1]:     # the smallest power of two >= 10 ms
            window *= 2
    w = _integer(window, "window")
    if w < ONSET_WINDOW_RANGE[0] or w > ONSET_WINDOW_RANGE[1] or w & (w - 1):
        raise ValueError("window must be a power of two in [%d, %d], got %d" % (ONSET_WINDOW_RANGE + (w,)))
    return w


def onset_plan(fs, window=None, bands=24, fmin=100.0):
    """What the bands kernel gets besides the signal (host only, no GPU): (win, k).
        win float64[w]: win[i] = 0.5 - 0.5 cos(2 pi (i + 0.5) / w); w = `window`, a power of two in [32, 2048], by default
            the smallest one >= 0.010 fs (256 at 16 kHz, 512 at 48 kHz)
        k int32[bands + 1]: band b holds the bins k[b] .. k[b + 1] - 1 of the w-point transform.  The edges are equally
            spaced on swipe.py's ERB scale between fmin and fs / 2; k[b] = ceil(edge_b w / fs), then k[b] = max(k[b],
            k[b - 1] + 1) so that no band is empty, then k[bands] = w / 2 + 1 (the last band holds the Nyquist bin).
    ValueError for fs <= 0, a window that is no power of two in range, bands outside [1, 64], fmin outside [0, fs / 2),
    and where the edges cannot be made strictly increasing (more bands than bins above fmin)."""
    fs = _sample_rate(fs)
    w = _window_length(fs, window)
    B = _in(bands, "bands", 1, ONSET_BANDS_MAX)
    fmin = _number(fmin, "fmin", 0)
    if not fmin < fs / 2:
        raise ValueError("fmin %g must lie below fs / 2 = %g" % (fmin, fs / 2))
    win = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(w) + 0.5) / w)
    edges = erbs2hz(np.linspace(hz2erbs(fmin), hz2erbs(fs / 2), B + 1))
    k = np.ceil(edges * w / fs).astype(np.int64)
    k[0] = max(k[0], 0)
    for b in range(1, B + 1):
        k[b] = max(k[b], k[b - 1] + 1)
    k[B] = w // 2 + 1
    if k[B - 1] >= k[B]:
        raise ValueError("%d bands above %g Hz do not fit the %d bins of a %d-sample window at fs = %g: no band may be "
                         "empty" % (B, fmin, w // 2 + 1, w, fs))
    return win, k.astype(np.int32)


def whole_frames(n, hop, window):
    """(first, last) frame all of whose `window` samples m hop - window/2 .. m hop + window/2 - 1 lie in [0, n);
    first > last where there is none."""
    half = window // 2
    first = -(-half // hop)
    last = (n - half) // hop if n >= half else -1
    return (first, last) if last >= first else (0, -1)


def check_onset_arguments(s, fs, hop=None, window=None, bands=24, fmin=100.0, lag=2, floor=1e-9):
    """Validates what onset_strength gets (no device work): returns (x float64[n], fs, hop, win, k, lag, floor).
    ValueError for s not 1-D, empty, not real numbers or not finite; fs <= 0; hop outside [1, 4096] (default
    round(0.005 fs)); lag outside [1, 16]; floor not finite and > 0; more than 2^31 - 1 frames; and whatever onset_plan
    refuses."""
    x = np.asarray(s)
    if x.ndim != 1 or x.dtype == object or not (np.issubdtype(x.dtype, np.number) or x.dtype == bool):
        raise ValueError("s must be a 1-D array of numbers")
    if np.iscomplexobj(x):
        raise ValueError("s must be real")
    x = np.ascontiguousarray(x, dtype=np.float64)
    if len(x) == 0:
        raise ValueError("s is empty")
    if not np.isfinite(x).all():
        raise ValueError("s must be finite")
    fs = _sample_rate(fs)
    hop = _in(int(round(0.005 * fs)) if hop is None else hop, "hop", 1, ONSET_HOP_MAX)
    win, k = onset_plan(fs, window, bands, fmin)
    lag = _in(lag, "lag", 1, ONSET_LAG_MAX)
    floor = _number(floor, "floor", above=0)
    if (len(x) - 1) // hop + 1 >= 2 ** 31:
        raise ValueError("s has %d frames at hop %d, 2^31 - 1 are possible" % ((len(x) - 1) // hop + 1, hop))
    return x, fs, hop, win, k, lag, floor


def onset_strength(s, fs, *, hop=None, window=None, bands=24, fmin=100.0, lag=2, floor=1e-9, return_bands=False,
                   device_index=0):
    """The onset strength of every frame of `s`: the spectral flux of the log band energies.
    Frame m of the Nf = (n - 1) // hop + 1 is the `window` samples around m hop (samples outside the signal are exact
    zeros), hop = round(0.005 fs) unless given: the noise model's frames.  L[m, b] = ln(E + floor) with E the energy of
    ERB band b (onset_plan), and d[m] = sum_b max(0, L[m, b] - L[m - lag, b]) / bands where m >= lag and frames m and
    m - lag both lie wholly inside the signal; d[m] is exactly 0 elsewhere, so neither the start nor the cut-off end of a
    file reads as an onset.  Returns dict(d float64[Nf], hop, window, fs, length); with return_bands=True also L
    float64[Nf, bands].  `s` is uploaded once and only the result comes back.  The same bits on every call."""
    x, fs, hop, win, k, lag, floor = check_onset_arguments(s, fs, hop, window, bands, fmin, lag, floor)
    device_index = _device_index(device_index)
    n, w, B = len(x), len(win), len(k) - 1
    Nf = (n - 1) // hop + 1
    lo, hi = whole_frames(n, hop, w)
    from .records import _device
    torch, c, dev = _device(device_index)
    L = torch.empty((Nf, B), dtype=torch.float64, device=dev)
    d = torch.empty(Nf, dtype=torch.float64, device=dev)
    sw = float(win.sum())
    c.onset_bands(torch.as_tensor(x, device=dev), n, w, hop, Nf, torch.as_tensor(win, device=dev), 1.0 / (sw * sw), k, B,
                  floor, L, B)
    c.onset_flux(L, Nf, B, B, lag, lo, hi, d)
    out = dict(d=d.cpu().numpy(), hop=hop, window=w, fs=fs, length=n)
    if return_bands:
        out["L"] = L.cpu().numpy()
    return out


# ---- the peaks
def check_strength(od):
    """Validates an onset strength (no device work): the dict onset_strength returns, d finite and >= 0 with
    1 <= len(d) < 2^31, hop an integer >= 1, fs > 0.  Returns (d float64[Nf] contiguous, hop, fs)."""
    if not isinstance(od, dict) or not all(key in od for key in ("d", "hop", "fs")):
        raise ValueError("an onset strength is the dict onset_strength returns: d, hop, fs")
    d = np.ascontiguousarray(_numeric_1d(od["d"], "d"))
    if not 1 <= len(d) < 2 ** 31:
        raise ValueError("d has %d frames, 1 to 2^31 - 1 are possible" % len(d))
    if not np.isfinite(d).all() or np.any(d < 0):
        raise ValueError("d must be finite and >= 0")
    hop = _integer(od["hop"], "hop")
    if hop < 1:
        raise ValueError("hop must be >= 1, got %d" % hop)
    return d, hop, _sample_rate(od["fs"])


def check_peak_arguments(delta=0.5, pre_max=3, post_max=3, pre_avg=20, post_avg=6, wait=10):
    """Validates the peak rule's parameters (no device work): delta finite and >= 0, the four windows integers in
    [0, 64], wait an integer >= 0.  Returns them in this order."""
    delta = _number(delta, "delta", 0)
    spans = tuple(_in(v, name, 0, ONSET_SPAN_MAX) for v, name in ((pre_max, "pre_max"), (post_max, "post_max"),
                                                                  (pre_avg, "pre_avg"), (post_avg, "post_avg")))
    wait = _integer(wait, "wait")
    if wait < 0:
        raise ValueError("wait must be >= 0, got %d" % wait)
    return (delta,) + spans + (wait,)


def keep_onsets(flagged, wait):
    """The `wait` rule over the flagged frames (ascending): after a KEPT frame the next `wait` frames are passed over, so
    a flagged frame m is dropped where m - last kept <= wait (Boeck's and librosa's reading of the rule).  Returns
    int64[K]."""
    kept = []
    for m in np.asarray(flagged, dtype=np.int64).tolist():
        if not kept or m - kept[-1] > wait:
            kept.append(m)
    return np.array(kept, dtype=np.int64)


def onsets(od, *, delta=0.5, pre_max=3, post_max=3, pre_avg=20, post_avg=6, wait=10, device_index=0):
    """The onsets of an onset strength (Boeck, Krebs and Schedl's rule).  Frame m is flagged on the
    device when d[m] > 0, d[m] is the maximum of d[m - pre_max .. m + post_max] and no earlier frame of that window
    equals it, and d[m] >= mean(d[m - pre_avg .. m + post_avg]) + delta, the windows cut at the ends.  On the host a
    flagged frame within `wait` frames of the last kept one is dropped (keep_onsets).  Returns dict(frames int64[K], times
    float64[K] = frames hop / fs in seconds, strength float64[K] = d[frames]).  The same bits on every call."""
    d, hop, fs = check_strength(od)
    delta, pre_max, post_max, pre_avg, post_avg, wait = check_peak_arguments(delta, pre_max, post_max, pre_avg, post_avg,
                                                                            wait)
    device_index = _device_index(device_index)
    from .records import _device
    torch, c, dev = _device(device_index)
    flag = torch.empty(len(d), dtype=torch.uint8, device=dev)
    c.onset_peaks(torch.as_tensor(d, device=dev), len(d), pre_max, post_max, pre_avg, post_avg, delta, flag)
    frames = keep_onsets(np.flatnonzero(flag.cpu().numpy()), wait)
    return dict(frames=frames, times=frames * hop / fs, strength=d[frames])


# ---- from onsets to a contour
def check_onset_times(times):
    """Onset times in seconds as float64[K] (no device work): 1-D, finite, >= 0; K may be 0."""
    t = _numeric_1d(np.zeros(0) if np.size(times) == 0 else times, "times")
    if not np.isfinite(t).all() or np.any(t < 0):
        raise ValueError("onset times must be finite and >= 0 (seconds)")
    return t


def _instants(DetComponents):
    from .records import _model_instants
    try:
        ti = _model_instants(DetComponents)
    except (TypeError, KeyError, AttributeError):
        raise ValueError("DetComponents must be a model: the structs or the arrays the analysis returns") from None
    if len(ti) < 2 or ti[0] != 0 or np.any(np.diff(ti) != ti[1] - ti[0]) or ti[1] <= 0:
        raise ValueError("the model's instants ti must start at sample 0 and be uniformly spaced, two at the least")
    return ti, int(ti[1])


def check_protection_arguments(DetComponents, fs, times, before=0.010, after=0.040, ramp=0.010):
    """Validates what protection_weight gets (no device work): returns (ti float64[No_ti] in samples, step, fs, times,
    before, after, ramp); before, after and ramp are finite and >= 0 (seconds)."""
    ti, step = _instants(DetComponents)
    return (ti, step, _sample_rate(fs), check_onset_times(times), _number(before, "before", 0),
            _number(after, "after", 0), _number(ramp, "ramp", 0))


def protection_weight(DetComponents, fs, times, *, before=0.010, after=0.040, ramp=0.010):
    """How much of every analysis instant is a transient (host only): p float64[No_ti] in [0, 1].  With
    t_i = ti / fs and, per onset, g = max(t_on - before - t_i, t_i - (t_on + after), 0) the distance to the plateau
    [t_on - before, t_on + after]: p_i = max over the onsets of max(0, 1 - g / ramp) (ramp = 0: 1 where g = 0, else 0).
    p is exactly 1 on every plateau and falls linearly to 0 over `ramp` on either side; without onsets it is 0."""
    ti, _, fs, times, before, after, ramp = check_protection_arguments(DetComponents, fs, times, before, after, ramp)
    t = ti / fs
    p = np.zeros(len(t))
    for t_on in times.tolist():
        g = np.maximum(np.maximum((t_on - before) - t, t - (t_on + after)), 0.0)
        p = np.maximum(p, (g == 0).astype(np.float64) if ramp == 0 else np.maximum(0.0, 1.0 - g / ramp))
    return p


def contour_length(r, step, length):
    """T(r) = step sum_j (r_j + r_{j+1}) / 2 + r_{n-1} (length - (n - 1) step): what contour_time_map rounds to L_out,
    linear in r."""
    r = np.asarray(r, dtype=np.float64)
    return float(step * ((r[:-1] + r[1:]) / 2).sum() + r[-1] * (length - (len(r) - 1) * step))


def protect_time_scale(DetComponents, fs, length, time_scale, times, *, before=0.010, after=0.040, ramp=0.010,
                       return_info=False):
    """The time-scale contour that leaves the transients at `times` alone (host only).  With rho the
    `time_scale` (a number, or a contour of one value per analysis instant) and p = protection_weight(...):
        rho'_i = p_i + (1 - p_i) c rho_i,   c = (T(rho) - T(p)) / T((1 - p) rho),   T = contour_length
    so the plateaus run at rate exactly 1, the rest is stretched by c times its own scale, and the total length is that
    of rho.  ValueError where T((1 - p) rho) <= 0 or c <= 0: nothing is left to stretch.  rho' is finally clipped to
    [0.25, 4]; where the clip acts the total length is approximate (as alignment_time_scale's is).  Returns rho'
    float64[No_ti] for eaQHMSynthesis(time_scale=); with return_info=True (rho', dict(c, clipped: the instants the clip
    changed, L_out: contour_time_map(rho', 1, step, length)["L_out"]))."""
    ti, step, fs, times, before, after, ramp = check_protection_arguments(DetComponents, fs, times, before, after, ramp)
    length = _integer(length, "length")
    if length < ti[-1] + 1:
        raise ValueError("length %d does not reach the model's last instant, sample %d" % (length, ti[-1]))
    rho = _contour(time_scale, "time_scale", len(ti))
    p = protection_weight(DetComponents, fs, times, before=before, after=after, ramp=ramp)
    rest = contour_length((1.0 - p) * rho, step, length)
    if not rest > 0:
        raise ValueError("every instant is protected: nothing is left to stretch")
    c = (contour_length(rho, step, length) - contour_length(p, step, length)) / rest
    if not c > 0:
        raise ValueError("the protected stretches alone are longer than the output (c = %g): nothing is left to stretch"
                         % c)
    raw = p + (1.0 - p) * (c * rho)
    out = np.clip(raw, *SCALE_RANGE)
    if not return_info:
        return out
    from .records import contour_time_map
    return out, dict(c=c, clipped=int(np.count_nonzero(out != raw)),
                     L_out=contour_time_map(out, np.ones(len(out)), step, length)["L_out"])
