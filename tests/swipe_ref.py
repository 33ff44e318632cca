"""The model of the device SWIPE' (eaqhm_amd.pitch -> eaqhm_swipe_*): a NumPy restatement of swipe.swipep stage by
stage, in float64 or in np.longdouble (the extended-precision FFT is scipy.fft.rfft), from the SAME float64 tables the
kernels get (pitch.swipe_plan).  No GPU and no library here.

    loudness(x, w, hop, pad, nframes, window, fs, lo, xlo, df, dtype) -> L [nframes, nE]
    scores(K, L, dtype) -> Si [cand, nframes]
    pick(windows, t, pc0, ntc, nftc, ptab, nf, dtype) -> dict(p, s, S, i, k, gap1, gap2)
    model(x, fs, plim, dtype) -> dict(track, L, Si, S, i, k, gap1, gap2, plan)
    decided(m, also=None) -> bool[T]

Decided instants.  The pitch of an instant follows from two maxima: over the candidates, then over the fine grid of the
winning candidate.  An implementation whose strengths are within rounding (a few 1e-15: the strengths are sums of
products of unit-norm rows) of the model's can differ in a maximum only where the best and the runner-up are closer than
that.  An instant is DECIDED when gap1 = best - runner-up over the candidates exceeds 1e-11 and, unless the maximum lies
on an edge candidate (no refinement), gap2 = best - runner-up over the fine grid does too: four orders above the rounding
of either side.  A column of exact zeros is decided by definition: argmax takes candidate 0, so p = pc[0], s = 0.
"""
import numpy as np

GAP = 1e-11
U = 2.0 ** -53


def _psd(xk, w, fs, window, hop, dtype):
    """swipe._psd_frames on the padded signal; the float64 run IS that function."""
    if dtype == np.float64:
        from eaqhm_amd.swipe import _psd_frames
        return _psd_frames(xk, w, fs, window, w - hop)[0]
    import scipy.fft
    nseg = (len(xk) - (w - hop)) // hop
    idx = np.arange(w)[:, None] + hop * np.arange(nseg)[None, :]
    seg = xk.astype(dtype)[idx] * window.astype(dtype)[:, None]
    spec = scipy.fft.rfft(seg, n=w, axis=0)
    assert spec.dtype == np.clongdouble
    psd = spec.real * spec.real + spec.imag * spec.imag
    psd[1:-1] *= dtype(2.0)
    psd /= dtype(fs)
    psd /= (np.abs(window.astype(dtype)) ** 2).sum()
    return psd


def loudness(x, w, hop, pad, nframes, window, fs, lo, xlo, df, dtype=np.float64):
    """L [nframes, nE]: frame m is the w samples of the zero-padded x from m hop - pad."""
    x = np.asarray(x, dtype=np.float64)
    total = (nframes - 1) * hop + w
    xk = np.zeros(total)
    a, b = max(0, -pad), min(len(x), total - pad)       # x[a:b] lands at pad + a
    if b > a:
        xk[pad + a:pad + b] = x[a:b]
    X = _psd(xk, w, fs, window, hop, dtype)             # (w/2 + 1, nframes)
    fp = X.T
    slope = (fp[..., lo + 1] - fp[..., lo]) / df.astype(dtype)
    Y = (slope * xlo.astype(dtype) + fp[..., lo]).T     # (nE, nframes)
    L = np.sqrt(np.maximum(0, Y))
    nrm = np.sqrt((L * L).sum(axis=0))
    nrm = np.where(nrm == 0, np.inf, nrm)
    return np.ascontiguousarray((L / nrm[None, :]).T)


def scores(K, L, dtype=np.float64):
    """Si [cand, nframes] = K . L^T; in float64 row by row, as swipe._strength_one forms it."""
    if dtype == np.float64:
        Lt = np.ascontiguousarray(L.T)
        return np.array([k @ Lt for k in K]).reshape(len(K), len(L))
    return K.astype(dtype) @ L.astype(dtype).T


def _interp(xp, fp, x):
    hi = np.clip(np.searchsorted(xp, x), 1, len(xp) - 1)
    lo = hi - 1
    slope = (fp[..., hi] - fp[..., lo]) / (xp[hi] - xp[lo])
    return slope * (x - xp[lo]) + fp[..., lo]


def pick(windows, t, npc, pc0, ntc, nftc, ptab, nf, dtype=np.float64):
    """`windows`: (Si [ncand, nframes], j0, mu [ncand], tshift [nframes]) in index order."""
    T = len(t)
    S = np.zeros((npc, T), dtype=dtype)
    td = t.astype(dtype)
    for Si, j0, mu, tshift in windows:
        v = _interp(tshift.astype(dtype), Si.astype(dtype), td)
        S[j0:j0 + len(mu)] = S[j0:j0 + len(mu)] + mu.astype(dtype)[:, None] * v
    best = S.argmax(axis=0)
    cols = np.arange(T)
    top = S[best, cols]
    rest = S.copy()
    rest[best, cols] = -np.inf
    gap1 = np.asarray(top - rest.max(axis=0), dtype=np.float64)
    p, s = np.full(T, np.nan), np.array(top, dtype=dtype)
    kbest, gap2 = np.full(T, -1), np.full(T, np.inf)
    edge = (best == 0) | (best == npc - 1)
    p[edge] = pc0
    for it in np.flatnonzero(~edge):
        i = best[it]
        x = ntc[i].astype(dtype)
        y = S[i - 1:i + 2, it]
        if dtype == np.float64:
            c = np.polyfit(x, y, 2)                       # swipep's own fit
        else:
            d01, d12 = (y[1] - y[0]) / (x[1] - x[0]), (y[2] - y[1]) / (x[2] - x[1])
            c2 = (d12 - d01) / (x[2] - x[0])
            c = (c2, d01 - c2 * (x[0] + x[1]), y[0] - x[0] * (d01 - c2 * x[1]))
        xf = nftc[i, :nf[i]].astype(dtype)
        val = np.zeros(len(xf), dtype=dtype)
        for ck in c:
            val = val * xf + ck
        k = int(val.argmax())
        others = np.delete(val, k)
        kbest[it], s[it], p[it] = k, val[k], ptab[i, k]
        gap2[it] = float(val[k] - others.max()) if len(others) else np.inf
    return dict(p=p, s=s, S=S, i=best, k=kbest, gap1=gap1, gap2=gap2)


def model(x, fs, plim, dtype=np.float64):
    from eaqhm_amd import pitch
    x, fs, plim = pitch.check_swipe_arguments(x, fs, plim)
    plan = pitch.swipe_plan(len(x), fs, plim)
    Ls, Sis, wins = [], [], []
    for w in plan["windows"]:
        L = loudness(x, w["w"], w["hop"], w["pad"], w["nframes"], w["window"], fs, w["lo"], w["xlo"], w["df"], dtype)
        Si = scores(w["K"], L, dtype)
        Ls.append(L)
        Sis.append(Si)
        wins.append((Si, w["j0"], w["mu"], w["tshift"]))
    out = pick(wins, plan["t"], len(plan["pc"]), plan["pc"][0], plan["ntc"], plan["nftc"], plan["ptab"], plan["nf"], dtype)
    out.update(track=np.column_stack((plan["t"], out["p"], np.asarray(out["s"], dtype=np.float64))), L=Ls, Si=Sis,
               plan=plan)
    return out


def decided(m, also=None):
    """bool[T] from one run of the model; with `also`, a second run (the other precision), a column counts as zero only
    where both runs have it exactly zero: a hand-made column that is zero up to the interpolation's rounding is a tie."""
    zero = ~np.asarray(m["S"] != 0).any(axis=0)
    if also is not None:
        zero &= ~np.asarray(also["S"] != 0).any(axis=0)
    return zero | ((m["gap1"] > GAP) & (m["gap2"] > GAP))


def bar(diff_models, scale=1.0):
    """The project's convention: 100 x the model's own float64-to-long-double difference, at least 64 u x the scale."""
    return max(100.0 * float(diff_models), 64 * U * scale)


def end_to_end_inputs():
    """The four inputs of the end-to-end tests: (name, x, fs, plim)."""
    import os
    from scipy.io import wavfile
    from eaqhm_amd.synth import synth_speech_int16
    here = os.path.dirname(os.path.abspath(__file__))
    fs, sa = wavfile.read(os.path.join(here, "golden", "SA19.WAV"))
    sa = sa / 32768.0
    return [("sa19", sa, fs, (160, 300)), ("sa19_1s_wide", sa[:fs], fs, (70, 500)),
            ("synth16k", synth_speech_int16(1.0, 16000) / 32768.0, 16000, (160, 300)),
            ("synth48k", synth_speech_int16(0.5, 48000) / 32768.0, 48000, (70, 500))]
