"""The model of the device's onset detector (eaqhm_amd.transient -> eaqhm_onset_*): DESIGN.md §15 in NumPy, stage by
stage, in float64 or in np.longdouble (the extended-precision FFT is scipy.fft.rfft), from the SAME float64 window and bin
edges the kernels get (transient.onset_plan).  No GPU and no library here.

    bands(x, w, hop, nframes, win, k, floor, dtype) -> L [nframes, B]
    flux(L, lag, whole_lo, whole_hi, dtype) -> d [nframes]
    peaks(d, pre_max, post_max, pre_avg, post_avg, delta) -> uint8 [nframes]
    model(x, fs, dtype=, fault=None, **options) -> dict(L, d, flag, frames, times, hop, window, k, win, whole)
    decided(m64, mld, bar_d, ...) -> bool[nframes]
    bar(diff_models, scale) -> the project's bar
    burst_signal(fs, seconds) -> (x, burst times): the synthetic signal of the tests

Flux and peaks are written in the kernels' order of operations (one addition after the other, ascending), so in float64
they are the kernels' bits.  `fault` plants one deliberate error (FAULTS) for the tests that show the bars can see it.

Decided flags.  A flag rests on comparisons between values of d: d[m] > 0, d[m] against every other frame of its
maximum window, d[m] against mean + delta.  Two implementations whose d agree within `bar_d` can differ in a comparison
only where its two sides are closer than 2 bar_d.  A comparison HOLDS decidedly when its margin exceeds 2 bar_d and FAILS
decidedly when it is missed by more than that; d[m] > 0 fails decidedly where both precisions have an exact zero and
holds decidedly above bar_d.  A flag is decided when every comparison holds decidedly, or one fails decidedly.
"""
import numpy as np

U = 2.0 ** -53
FAULTS = ("window_half", "kB_short", "lag_minus", "no_whole", "ties_last")


def bar(diff_models, scale=1.0):
    """The project's convention: 100 x the model's own float64-to-long-double difference, at least 64 u x the scale."""
    return max(100.0 * float(diff_models), 64 * U * max(1.0, float(scale)))


def frames_of(x, w, hop, nframes, dtype=np.float64):
    """[nframes, w]: frame m is x[m hop - w/2 .. m hop + w/2 - 1], exact zeros outside the signal."""
    x = np.asarray(x, dtype=np.float64)
    idx = (np.arange(nframes, dtype=np.int64) * hop - w // 2)[:, None] + np.arange(w)[None, :]
    inside = (idx >= 0) & (idx < len(x))
    return np.where(inside, x[np.clip(idx, 0, len(x) - 1)], 0.0).astype(dtype)


def bands(x, w, hop, nframes, win, k, floor, dtype=np.float64):
    k = np.asarray(k, dtype=np.int64)
    seg = frames_of(x, w, hop, nframes, dtype) * win.astype(dtype)[None, :]
    if dtype == np.float64:
        X = np.fft.rfft(seg, n=w, axis=1)
        sw = float(win.sum())                       # the host's own expression: the kernel gets this double
        inv = 1.0 / (sw * sw)
    else:
        import scipy.fft
        X = scipy.fft.rfft(seg, n=w, axis=1)
        assert X.dtype == np.clongdouble
        sw = win.astype(dtype).sum()
        inv = dtype(1.0) / (sw * sw)
    P = (X.real * X.real + X.imag * X.imag) * inv
    E = np.zeros((nframes, len(k) - 1), dtype=dtype)
    for b in range(len(k) - 1):
        for kk in range(k[b], k[b + 1]):            # ascending, one addition after the other
            E[:, b] = E[:, b] + P[:, kk]
    return np.log(E + dtype(floor))


def flux(L, lag, whole_lo, whole_hi, dtype=np.float64):
    L = np.asarray(L, dtype=dtype)
    nframes, B = L.shape
    d = np.zeros(nframes, dtype=dtype)
    m = np.arange(nframes)
    on = (m >= lag) & (m - lag >= whole_lo) & (m <= whole_hi)
    at = m[on]
    acc = np.zeros(len(at), dtype=dtype)
    for b in range(B):
        acc = acc + np.maximum(L[at, b] - L[at - lag, b], dtype(0))
    d[at] = acc / dtype(B)
    return d


def peaks(d, pre_max=3, post_max=3, pre_avg=20, post_avg=6, delta=0.5, ties_last=False):
    d = np.asarray(d)
    n = len(d)
    flag = np.zeros(n, dtype=np.uint8)
    for m in range(n):
        v = d[m]
        if not v > 0:
            continue
        before, after = d[max(0, m - pre_max):m], d[m + 1:min(n - 1, m + post_max) + 1]
        if ties_last:
            if (before > v).any() or (after >= v).any():
                continue
        elif (before >= v).any() or (after > v).any():
            continue
        acc = d.dtype.type(0)
        a0, a1 = max(0, m - pre_avg), min(n - 1, m + post_avg)
        for j in range(a0, a1 + 1):
            acc = acc + d[j]
        if v >= acc / d.dtype.type(a1 - a0 + 1) + d.dtype.type(delta):
            flag[m] = 1
    return flag


def model(x, fs, dtype=np.float64, fault=None, *, hop=None, window=None, bands_=24, fmin=100.0, lag=2, floor=1e-9,
          delta=0.5, pre_max=3, post_max=3, pre_avg=20, post_avg=6, wait=10):
    """The whole detector on the host, from transient's own plan and checks."""
    from eaqhm_amd import transient
    assert fault is None or fault in FAULTS
    x, fs, hop, win, k, lag, floor = transient.check_onset_arguments(x, fs, hop, window, bands_, fmin, lag, floor)
    w = len(win)
    nframes = (len(x) - 1) // hop + 1
    lo, hi = transient.whole_frames(len(x), hop, w)
    if fault == "window_half":
        win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(w) / w)
    if fault == "kB_short":
        k = k.copy()
        k[-1] -= 1
    if fault == "no_whole":
        lo, hi = 0, nframes - 1
    L = bands(x, w, hop, nframes, win, k, floor, dtype)
    d = flux(L, lag - 1 if fault == "lag_minus" else lag, lo, hi, dtype)
    flag = peaks(d, pre_max, post_max, pre_avg, post_avg, delta, ties_last=fault == "ties_last")
    frames = transient.keep_onsets(np.flatnonzero(flag), wait)
    return dict(L=L, d=d, flag=flag, frames=frames, times=frames * hop / fs, hop=hop, window=w, k=k, win=win,
                whole=(lo, hi), fs=fs, length=len(x))


def decided(m64, mld, bar_d, pre_max=3, post_max=3, pre_avg=20, post_avg=6, delta=0.5):
    """bool[nframes] from the two runs of the model (float64 and long double) and the bar on d."""
    d, dl = np.asarray(mld["d"], dtype=np.float64), np.asarray(m64["d"], dtype=np.float64)
    n = len(d)
    out = np.zeros(n, dtype=bool)
    g = 2.0 * bar_d
    for m in range(n):
        v = d[m]
        if v == 0 and dl[m] == 0:
            out[m] = True                                   # d[m] > 0 fails in both precisions, exactly
            continue
        others = np.concatenate((d[max(0, m - pre_max):m], d[m + 1:min(n - 1, m + post_max) + 1]))
        a0, a1 = max(0, m - pre_avg), min(n - 1, m + post_avg)
        s = v - (d[a0:a1 + 1].sum() / (a1 - a0 + 1) + delta)
        fails = (len(others) and (others - v).max() > g) or s < -g
        holds = v > bar_d and (not len(others) or (v - others).min() > g) and s > g
        out[m] = bool(fails or holds)
    return out


def burst_signal(fs, seconds=2.0, seed=0):
    """The synthetic signal of the tests: ten harmonics of 200 Hz with amplitudes 0.2 / h, 3 % vibrato at 5 Hz and 20 %
    tremolo at 3 Hz, white noise at 1e-3, and 5 ms white bursts of amplitude 0.3, 0.1, 0.3, 0.1 at 0.4, 0.9, 1.3 and
    1.7 s (those that fit).  Returns (x float64[round(seconds fs)], the burst times)."""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * fs))
    t = np.arange(n) / float(fs)
    phase = 2 * np.pi * 200.0 * (t - 0.03 / (2 * np.pi * 5.0) * np.cos(2 * np.pi * 5.0 * t))   # f = 200 (1 + .03 sin)
    x = np.zeros(n)
    for h in range(1, 11):
        x += 0.2 / h * np.sin(h * phase)
    x *= 1.0 + 0.2 * np.sin(2 * np.pi * 3.0 * t)
    x += 1e-3 * rng.standard_normal(n)
    times = []
    for t_on, amp in ((0.4, 0.3), (0.9, 0.1), (1.3, 0.3), (1.7, 0.1)):
        a, b = int(round(t_on * fs)), int(round((t_on + 0.005) * fs))
        if b <= n:
            x[a:b] += amp * rng.standard_normal(b - a)
            times.append(t_on)
    return x, np.array(times)


def sa19():
    """(x, fs): the recorded sentence of tests/golden."""
    import os
    from scipy.io import wavfile
    fs, x = wavfile.read(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "SA19.WAV"))
    return x / 32768.0, fs
