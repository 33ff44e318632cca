"""Transient onsets on the MI355X (eaqhm_amd.transient -> eaqhm_onset_bands / _flux / _peaks) against tests/transient_ref.py,
the NumPy model of DESIGN.md §15 in float64 and long double.

Bars.  Band energies and the flux of a signal: max(100 x the model's own float64-to-long-double difference on that case,
64 u x max(1, the largest |value|)), against the long-double model.  Flux and peaks on hand-made inputs: the model's bits
(the model adds in the kernels' order).  Flags of a signal: equal on every decided frame (transient_ref.decided).  Every
test prints the device's error as a fraction of its bar."""
import os

import numpy as np
import pytest

import transient_ref as R
from conftest import GOLDEN, load_golden, record_measurement

pytestmark = pytest.mark.gpu

LD = np.longdouble
FLOOR = 1e-9
WORST = {}


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


def ctx():
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    return torch, c, c.device


def up(a):
    torch, _, d = ctx()
    return torch.as_tensor(np.ascontiguousarray(a), device=d)


def window(w):
    return 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(w) + 0.5) / w)


def inv_sumw2(win):
    sw = float(win.sum())
    return 1.0 / (sw * sw)


def worst(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


# ---- 1. the band energies
def gpu_bands(x, w, hop, nframes, win, k, ld=None, floor=FLOOR):
    torch, c, d = ctx()
    B = len(k) - 1
    ld = B if ld is None else ld
    L = torch.full((nframes + 2, ld), np.nan, dtype=torch.float64, device=d)
    c.onset_bands(up(x), len(x), w, hop, nframes, up(win), inv_sumw2(win), k, B, floor, L[:nframes], ld)
    out = L.cpu().numpy()
    assert np.isnan(out[nframes:]).all() and np.isnan(out[:nframes, B:]).all()           # nothing beyond the cells
    return out[:nframes, :B]


def edges(w, B):
    """Bin edges of B bands of a w-point transform; 24: the plan's own at 16 kHz where it fits."""
    nb = w // 2 + 1
    if B == 1:
        return np.array([0, nb], dtype=np.int32)                             # DC to Nyquist in one band
    if B == 2:
        return np.array([3, nb - 1, nb], dtype=np.int32)                     # the second band is the Nyquist bin alone
    if B == 24 and w >= 128:
        from eaqhm_amd import transient
        return transient.onset_plan(16000, w, 24, 100.0)[1]
    B = min(B, nb)                                                           # one-bin bands, the last takes the rest
    return np.concatenate((np.arange(B), [nb])).astype(np.int32)


def signal(kind, n, w, hop, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.standard_normal(n) * np.exp(-np.arange(n) / (n + 1.0))
    if kind == "sinusoid":
        return 0.7 * np.sin(2 * np.pi * 0.1037 * np.arange(n) + 0.4)
    if kind == "zeros":
        return np.zeros(n)
    if kind == "constant":
        return np.full(n, 0.75)
    x = np.zeros(n)                                                          # impulse
    x[min(n - 1, (n // 2 // hop) * hop + (w // 8 if hop > 1 else 0))] = 1.0
    return x


def band_cases(w):
    """(hop, Nf, extra samples beyond the last frame centre, B, signal, padded row)."""
    return [(1, 65, 0, 24, "noise", False),                  # n = 65: for w >= 256 no frame is whole
            (w // 4, 65, w // 4 - 1, 64, "sinusoid", True),
            (w // 4, 65, 3, 24, "impulse", False),
            (w // 4, 65, 0, 64, "noise", False),
            (w, 3, w // 2 + 5, 2, "constant", True),
            (w, 3, 1, 2, "noise", False),
            (3 * w // 2, 2, 7, 1, "zeros", False),
            (3 * w // 2, 2, 7, 24, "noise", True),
            (w // 4, 1, w // 4 - 1, 1, "noise", False),       # n < w: one cut-off frame
            (w, 1, 0, 2, "impulse", False)]                   # n = 1


BANDS = [(w,) + c for w in (32, 64, 256, 512, 2048) for c in band_cases(w)]


@pytest.mark.parametrize("w,hop,nframes,extra,B,kind,padded", BANDS,
                         ids=["w%d-hop%d-nf%d+%d-B%d-%s%s" % (c[:6] + ("-ld" if c[6] else "",)) for c in BANDS])
def test_bands_direct(amd, w, hop, nframes, extra, B, kind, padded):
    n = (nframes - 1) * hop + 1 + extra
    assert (n - 1) // hop + 1 == nframes
    x = signal(kind, n, w, hop, seed=w + hop + B)
    win, k = window(w), edges(w, B)
    nB = len(k) - 1
    ld = nB + 3 if padded else None
    got = gpu_bands(x, w, hop, nframes, win, k, ld)
    again = gpu_bands(x, w, hop, nframes, win, k, ld)
    m64, mld = R.bands(x, w, hop, nframes, win, k, FLOOR), R.bands(x, w, hop, nframes, win, k, FLOOR, LD)
    bar = R.bar(np.abs(m64 - mld).max(), np.abs(mld).max())
    err = float(np.abs(got - mld).max())
    print("bands w=%d hop=%d nf=%d B=%d %s: error / bar %.3g (bar %.2e)" % (w, hop, nframes, nB, kind, err / bar, bar))
    record_measurement("onset_bands_w%d_hop%d_nf%d_B%d_%s" % (w, hop, nframes, nB, kind), err_over_bar=err / bar, bar=bar)
    worst("bands", err / bar)
    assert got.view(np.int64).tolist() == again.view(np.int64).tolist()      # the same bits on every call
    assert np.isfinite(got).all() and err <= bar
    if kind == "zeros":
        assert len(np.unique(got.view(np.int64))) == 1 and abs(got[0, 0] - np.log(FLOOR)) <= bar
    if kind == "impulse":                                                    # |X_k|^2 = win[pos]^2 at every bin
        at = int(np.flatnonzero(x)[0])
        pos = at - (np.arange(nframes) * hop - w // 2)                       # the impulse's place in every frame
        inside = (pos >= 0) & (pos < w)
        assert inside.any()
        amp = np.where(inside, win[np.clip(pos, 0, w - 1)], 0.0).astype(LD)
        closed = np.log(np.diff(k).astype(LD)[None, :] * (amp * amp)[:, None] * LD(inv_sumw2(win)) + LD(FLOOR))
        assert np.abs(got - closed).max() <= bar
        dark = got[~inside].view(np.int64)                                   # frames without the impulse: ln(floor)
        assert not len(dark) or (len(np.unique(dark)) == 1 and abs(got[~inside][0, 0] - np.log(FLOOR)) <= bar)


@pytest.mark.parametrize("w", [32, 64, 256, 512, 2048])
def test_bands_position_independent(amd, w):
    """The same w samples give the same bits wherever the frame sits in the launch and whatever its neighbours are."""
    rng = np.random.default_rng(w)
    hop, win, k = w // 4, window(w), edges(w, 24)
    chunk = rng.standard_normal(w)
    rows = []
    for seed, nframes, places in ((1, 40, (7, 12)), (2, 23, (2, 20)), (3, 9, (5,))):
        x = np.random.default_rng(seed).standard_normal((nframes - 1) * hop + 1)
        for m in places:
            x[m * hop - w // 2:m * hop + w // 2] = chunk
        got = gpu_bands(x, w, hop, nframes, win, k)
        rows += [got[m] for m in places]
        others = np.delete(got, places, axis=0)
        assert not (others == got[places[0]]).all(axis=1).any()              # the neighbours are other frames
    alone = gpu_bands(np.concatenate((np.zeros(w // 2), chunk)), w, w, 2, win, k)[1]   # zeros before, nothing after
    rows.append(alone)
    bits = np.array(rows).view(np.int64)
    assert (bits == bits[0]).all()


def test_bands_refuses(amd):
    torch, c, d = ctx()
    w, B = 64, 4
    win, k = window(w), [1, 2, 5, 9, 33]
    x = up(np.ones(200))
    L = torch.full((4, B), np.nan, dtype=torch.float64, device=d)
    good = dict(x=x, n=200, w=w, hop=16, nframes=4, window=up(win), inv_sumw2=1.0, k=k, B=B, floor=FLOOR, L=L, ld=B)
    for kw in (dict(w=48), dict(w=16), dict(w=4096), dict(hop=0), dict(hop=4097), dict(nframes=0), dict(nframes=2 ** 31),
               dict(n=0), dict(B=0, k=[1]), dict(B=65, k=list(range(66))), dict(ld=3), dict(k=[1, 2, 2, 9, 33]),
               dict(k=[1, 2, 5, 9, 34]), dict(k=[-1, 2, 5, 9, 33]), dict(floor=0.0), dict(floor=float("nan")),
               dict(inv_sumw2=0.0), dict(inv_sumw2=float("inf")), dict(x=None), dict(window=None), dict(L=None)):
        args = dict(good)
        args.update(kw)
        with pytest.raises(RuntimeError, match="eaqhm_onset_bands"):
            c.onset_bands(**args)
    c.sync()
    assert np.isnan(L.cpu().numpy()).all()                                   # no output touched
    c.onset_bands(**good)
    assert np.isfinite(L.cpu().numpy()).all()


# ---- 2. the flux, on hand-made band energies: the model's bits
def gpu_flux(L, B, lag, lo, hi):
    torch, c, d = ctx()
    nframes, ld = L.shape
    out = torch.full((nframes + 2,), np.nan, dtype=torch.float64, device=d)
    c.onset_flux(up(L), nframes, ld, B, lag, lo, hi, out[:nframes])
    got = out.cpu().numpy()
    assert np.isnan(got[nframes:]).all()
    return got[:nframes]


FLUX = [(nf, B, lag) for nf in (1, 2, 17, 300) for B, lag in ((1, 1), (24, 2), (64, 16), (3, 1))]


@pytest.mark.parametrize("nframes,B,lag", FLUX, ids=["nf%d-B%d-lag%d" % c for c in FLUX])
def test_flux_bits(amd, nframes, B, lag):
    rng = np.random.default_rng(nframes + B)
    ld = B + (2 if B == 24 else 0)
    L = np.round(rng.normal(-10, 4, (nframes, ld)), 1)                        # coarse values: equal cells occur
    L[:, B:] = 1e300                                                         # never read
    if nframes > 20:
        L[10:14] = L[9]                                                      # a plateau: differences of exactly 0
    for lo, hi in ((0, nframes - 1), (2, nframes - 3), (5, 4), (0, -1), (nframes - 1, nframes - 1), (-3, nframes + 5)):
        got = gpu_flux(L, B, lag, lo, hi)
        want = R.flux(L[:, :B], lag, lo, hi)
        assert got.view(np.int64).tolist() == want.view(np.int64).tolist(), (lo, hi)
        assert not got[:lag].any() and (hi >= lo or not got.any())
    if nframes > 20:
        full = gpu_flux(L, B, lag, 0, nframes - 1)
        assert full[lag:].any() and (full >= 0).all()
        if lag == 1:
            assert not full[10:14].any()


def test_flux_refuses(amd):
    torch, c, d = ctx()
    L = up(np.zeros((5, 4)))
    out = torch.full((5,), np.nan, dtype=torch.float64, device=d)
    good = dict(L=L, nframes=5, ld=4, B=4, lag=2, whole_lo=0, whole_hi=4, d=out)
    for kw in (dict(lag=0), dict(lag=17), dict(B=0), dict(B=65, ld=65), dict(ld=3), dict(nframes=0), dict(nframes=2 ** 31),
               dict(L=None), dict(d=None)):
        args = dict(good)
        args.update(kw)
        with pytest.raises(RuntimeError, match="eaqhm_onset_flux"):
            c.onset_flux(**args)
    c.sync()
    assert np.isnan(out.cpu().numpy()).all()


# ---- 3. the peaks, on hand-made strengths: the model's bits
def gpu_peaks(dv, pre_max, post_max, pre_avg, post_avg, delta):
    torch, c, d = ctx()
    n = len(dv)
    flag = torch.full((n + 3,), 7, dtype=torch.uint8, device=d)
    c.onset_peaks(up(np.asarray(dv, dtype=np.float64)), n, pre_max, post_max, pre_avg, post_avg, delta, flag[:n])
    got = flag.cpu().numpy()
    assert (got[n:] == 7).all()
    return got[:n]


def strengths(kind, n):
    rng = np.random.default_rng(n)
    if kind == "plateaus":
        return np.repeat(rng.integers(0, 4, n // 3 + 1) / 2.0, 3)[:n]        # runs of three equal values, zeros among them
    if kind == "zeros":
        return np.zeros(n)
    if kind == "ramp":
        return np.arange(n) / 8.0
    d = np.abs(rng.standard_normal(n)) * (rng.uniform(size=n) < 0.3)
    d[rng.integers(0, n, max(1, n // 10))] += 3.0
    return d


PEAK_PARAMS = [(3, 3, 20, 6, 0.5), (0, 0, 0, 0, 0.0), (64, 64, 64, 64, 0.0), (0, 64, 64, 0, 0.25), (64, 0, 0, 64, 0.5),
               (1, 2, 3, 4, 0.0)]
PEAKS = [(kind, n) for kind in ("plateaus", "zeros", "ramp", "sparse") for n in (1, 5, 130, 1000)]


@pytest.mark.parametrize("kind,n", PEAKS, ids=["%s-%d" % c for c in PEAKS])
def test_peaks_bits(amd, kind, n):
    d = strengths(kind, n)
    flagged = 0
    for params in PEAK_PARAMS:
        got = gpu_peaks(d, *params)
        want = R.peaks(d, *params)
        assert got.tolist() == want.tolist(), params
        flagged += int(got.sum())
    if kind == "zeros":
        assert flagged == 0
    elif n >= 130:
        assert flagged > 0
    if kind == "plateaus" and n >= 130:                                      # ties go to the first of a run
        got = np.flatnonzero(gpu_peaks(d, 1, 1, 0, 0, 0.0))
        assert len(got) and all(m == 0 or d[m - 1] < d[m] for m in got)


def test_peaks_refuses(amd):
    torch, c, d = ctx()
    dv = up(np.ones(6))
    flag = torch.full((6,), 7, dtype=torch.uint8, device=d)
    good = dict(d=dv, nframes=6, pre_max=3, post_max=3, pre_avg=20, post_avg=6, delta=0.5, flag=flag)
    for kw in (dict(pre_max=-1), dict(pre_max=65), dict(post_max=-1), dict(post_max=65), dict(pre_avg=-1), dict(pre_avg=65),
               dict(post_avg=-1), dict(post_avg=65), dict(delta=-0.5), dict(delta=float("nan")), dict(delta=float("inf")),
               dict(nframes=0), dict(nframes=2 ** 31), dict(d=None), dict(flag=None)):
        args = dict(good)
        args.update(kw)
        with pytest.raises(RuntimeError, match="eaqhm_onset_peaks"):
            c.onset_peaks(**args)
    c.sync()
    assert (flag.cpu().numpy() == 7).all()


# ---- 4. end to end
def signals():
    x19, fs19 = R.sa19()
    return [("burst16k",) + R.burst_signal(16000, 1.0) + (16000,), ("burst48k",) + R.burst_signal(48000, 1.0) + (48000,),
            ("sa19", x19, None, fs19)]


@pytest.mark.parametrize("name", ["burst16k", "burst48k", "sa19"])
def test_end_to_end(amd, name):
    from eaqhm_amd import transient
    _, x, bursts, fs = [s for s in signals() if s[0] == name][0]
    od = transient.onset_strength(x, fs, return_bands=True)
    again = transient.onset_strength(x, fs)
    m64, mld = R.model(x, fs), R.model(x, fs, LD)
    assert (od["hop"], od["window"], od["length"], len(od["d"])) == (m64["hop"], m64["window"], len(x), len(m64["d"]))
    assert od["d"].view(np.int64).tolist() == again["d"].view(np.int64).tolist() and "L" not in again
    bar_L = R.bar(np.abs(m64["L"] - mld["L"]).max(), np.abs(mld["L"]).max())
    bar_d = R.bar(np.abs(m64["d"] - mld["d"]).max(), np.abs(mld["d"]).max())
    err_L, err_d = float(np.abs(od["L"] - mld["L"]).max()), float(np.abs(od["d"] - mld["d"]).max())
    print("%s: L error / bar %.3g (bar %.2e), d error / bar %.3g (bar %.2e)" % (name, err_L / bar_L, bar_L, err_d / bar_d,
                                                                               bar_d))
    record_measurement("onset_end_to_end_" + name, L_err_over_bar=err_L / bar_L, d_err_over_bar=err_d / bar_d, bar_d=bar_d)
    worst("bands", err_L / bar_L)
    worst("flux", err_d / bar_d)
    assert err_L <= bar_L and err_d <= bar_d
    lo, hi = m64["whole"]
    assert not od["d"][:lo + 2].any() and not od["d"][hi + 1:].any()         # exact zeros where the model has them
    flag = gpu_peaks(od["d"], 3, 3, 20, 6, 0.5)
    dec = R.decided(m64, mld, bar_d)
    print("%s: %d of %d flags decided, %d flagged" % (name, dec.sum(), len(dec), flag.sum()))
    assert dec.mean() > 0.99 and np.array_equal(flag[dec], mld["flag"][dec])
    on = transient.onsets(od)
    assert np.array_equal(on["frames"], m64["frames"]) and on["frames"].dtype == np.int64
    assert np.array_equal(on["times"], on["frames"] * od["hop"] / float(fs))
    assert np.array_equal(on["strength"], od["d"][on["frames"]])
    if bursts is not None:
        assert len(on["frames"]) == len(bursts) == 2
        assert np.abs(on["frames"] - bursts * fs / od["hop"]).max() <= 1    # within one frame of its burst
    else:
        assert 12 <= len(on["frames"]) <= 32


def test_options_reach_the_kernels(amd):
    """hop, window, bands, fmin, lag and floor as arguments, and the peak rule's parameters, against the model."""
    from eaqhm_amd import transient
    x, _ = R.burst_signal(16000, 1.0)
    opts = dict(hop=100, window=512, fmin=300.0, lag=3, floor=1e-6)
    od = transient.onset_strength(x, 16000, bands=16, return_bands=True, **opts)
    m64, mld = R.model(x, 16000, bands_=16, **opts), R.model(x, 16000, LD, bands_=16, **opts)
    assert od["L"].shape == (160, 16) and od["hop"] == 100 and od["window"] == 512
    bar_d = R.bar(np.abs(m64["d"] - mld["d"]).max(), np.abs(mld["d"]).max())
    err = float(np.abs(od["d"] - mld["d"]).max())
    worst("flux", err / bar_d)
    assert err <= bar_d
    peak = dict(delta=0.2, pre_max=5, post_max=1, pre_avg=10, post_avg=2, wait=4)
    on = transient.onsets(od, **peak)
    want = transient.keep_onsets(np.flatnonzero(R.peaks(od["d"], 5, 1, 10, 2, 0.2)), 4)
    assert np.array_equal(on["frames"], want) and len(want) >= 2


# ---- 5. the protected contour through the synthesis
def test_protected_synthesis(amd):
    from eaqhm_amd import transient
    from test_gpu_model_synthesis import reference_model
    g, det = reference_model()
    fs, s = amd.read_signal(os.path.join(GOLDEN, "SA19.WAV"))
    length = len(g["s_recon"])
    assert fs == 16000 and len(s) == length
    on = transient.onsets(transient.onset_strength(s, fs))
    p = transient.protection_weight(det, fs, on["times"])
    rho, info = transient.protect_time_scale(det, fs, length, 2.0, on["times"], return_info=True)
    assert 12 <= len(on["times"]) <= 32 and p.mean() < 0.4 and info["clipped"] == 0 and abs(info["L_out"] - 2 * length) <= 1
    noise = amd.eaQHMNoiseAnalysis(s, g["s_recon"], fs)
    y = amd.eaQHMSynthesis(det, fs, length, time_scale=rho, phase="shape", noise=noise)
    print("SA19 at 2 x with %d protected transients: c = %.4f, %d samples" % (len(on["times"]), info["c"], len(y)))
    assert y.dtype == np.float64 and y.shape == (info["L_out"],) and np.isfinite(y).all() and np.abs(y).max() > 1e-3


def test_report_worst():
    """The largest error seen as a fraction of its bar (runs last: the tests above fill the table)."""
    print("largest error / bar: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))
    record_measurement("onset_worst_error_over_bar", **WORST)
    assert WORST and max(WORST.values()) <= 1.0
