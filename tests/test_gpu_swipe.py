"""SWIPE' on the MI355X (eaqhm_amd.pitch -> eaqhm_swipe_loudness / _scores / _pick) against tests/swipe_ref.py, the NumPy
model in float64 and long double that tests/test_swipe_device_cpu.py ties to swipe.swipep, and against swipep itself.

Bars.  Unless a test says otherwise: max(100 x the model's own float64-to-long-double difference on that case, 64 u x the
quantity's scale); loudness rows have norm 1 and strengths are at most about 1, so the scale is 1.  Scores: twice the
worst-case bound nE u (|K| |L|^T), entry by entry, against the long-double product.  Decisions (the candidate, the
fine-grid point, hence the pitch, which is read from the host's table) are equal on every decided instant
(swipe_ref.decided).  Every test prints the device's error as a fraction of its bar."""
import os

import numpy as np
import pytest

import swipe_ref as R
from conftest import GOLDEN, load_golden, record_measurement

pytestmark = pytest.mark.gpu

LD = np.longdouble
FS = 16000.0


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


# ---- 1. loudness
def erb_tables(w, nE, seed):
    """nE ascending frequencies inside (0, fs / 2), one of them exactly a bin frequency, and swipe_plan's tables for them."""
    rng = np.random.default_rng(seed)
    f = np.arange(w // 2 + 1) * (FS / w)
    fe = np.sort(rng.uniform(FS / w / 4, FS / 2 * 0.999, nE))
    fe[nE // 2] = f[max(1, min(len(f) - 2, np.searchsorted(f, fe[nE // 2])))]
    fe = np.sort(fe)
    hi = np.clip(np.searchsorted(f, fe), 1, len(f) - 1)
    lo = hi - 1
    assert np.any(fe == f[hi])                                              # the point on a bin
    return lo.astype(np.int32), fe - f[lo], f[hi] - f[lo]


def gpu_loudness(x, w, hop, pad, nframes, window, lo, xlo, df, ld=None):
    torch, c, d = ctx()
    nE = len(lo)
    ld = nE if ld is None else ld
    L = torch.full((nframes + 2, ld), np.nan, dtype=torch.float64, device=d)
    sumw2 = float((np.abs(window) ** 2).sum())
    c.swipe_loudness(up(x), len(x), w, hop, pad, nframes, up(window), FS, sumw2, up(lo), up(xlo), up(df), nE, L[:nframes], ld)
    out = L.cpu().numpy()
    assert np.isnan(out[nframes:]).all() and np.isnan(out[:nframes, nE:]).all()          # nothing beyond the rows
    return out[:nframes, :nE]


def loudness_case(w, kind, nE, seed):
    """(x, hop, pad, nframes): `kind` is the frame count (2: n = 5; 3; 65) or a named signal over 65 frames."""
    rng = np.random.default_rng(seed)
    hop, pad = w // 2, w // 2
    if kind == 2:
        return rng.standard_normal(5), hop, pad, 2
    if kind == 3:
        return rng.standard_normal(hop + 3), hop, pad, 3
    n = 63 * hop + 7                                                         # 65 frames: the last holds 7 samples
    if kind == "zeros":
        x = rng.standard_normal(n)
        x[10 * hop + 1:17 * hop] = 0.0                                       # a run of exact zeros longer than 2 w
    elif kind == "constant":
        x = np.full(n, 0.75)
    elif kind == "impulse":
        x = np.zeros(n)
        x[20 * hop + hop // 3] = 1.0
    else:
        x = rng.standard_normal(n) * np.exp(-np.arange(n) / n)
    return x, hop, pad, 65


LOUD = [(w, kind, nE) for w in (8, 64, 256, 1024, 8192)
        for kind, nE in ((2, 1), (3, 63), (65, 64), (65, 65), ("zeros", 318), ("constant", 65), ("impulse", 64))]


@pytest.mark.parametrize("w,kind,nE", LOUD, ids=["w%d-%s-nE%d" % c for c in LOUD])
def test_loudness_direct(amd, w, kind, nE):
    x, hop, pad, nframes = loudness_case(w, kind, nE, seed=w + nE)
    lo, xlo, df = erb_tables(w, nE, seed=nE)
    window = np.hanning(w)
    m64 = R.loudness(x, w, hop, pad, nframes, window, FS, lo, xlo, df)
    mld = R.loudness(x, w, hop, pad, nframes, window, FS, lo, xlo, df, LD)
    ld = nE + 3 if kind == 65 else None
    got = gpu_loudness(x, w, hop, pad, nframes, window, lo, xlo, df, ld)
    again = gpu_loudness(x, w, hop, pad, nframes, window, lo, xlo, df, ld)
    bar = R.bar(np.abs(m64 - mld).max())
    err = float(np.abs(got - mld).max())
    print("loudness w=%d %s nE=%d: error / bar %.3g (bar %.2e)" % (w, kind, nE, err / bar, bar))
    record_measurement("swipe_loudness_w%d_%s_%d" % (w, kind, nE), err_over_bar=err / bar, bar=bar)
    assert np.array_equal(got, again)
    assert err <= bar
    silent = ~mld.any(axis=1)
    assert not got[silent].any()                                             # a frame of zeros: an exactly zero row
    norms = np.sqrt((got[~silent].astype(LD) ** 2).sum(axis=1))
    assert np.abs(norms - 1).max() <= 64 * R.U if len(norms) else True
    if kind == "zeros":
        start = np.arange(nframes) * hop - pad
        inside = (start >= 10 * hop + 1) & (start + w <= 17 * hop)
        assert inside.sum() >= 3 and silent[inside].all()
    if kind == "impulse":                                                    # |X_k|^2 = window[i]^2 at every bin
        lit = np.flatnonzero(~silent)
        inner = (lo >= 1) & (lo + 1 < w // 2)
        assert len(lit) in (1, 2)
        if inner.sum() > 1:
            rows = got[lit][:, inner]
            assert np.abs(rows - rows[:, :1]).max() <= bar


def test_loudness_uneven_hop(amd):
    """hop and pad that are not half the window, frames that start before and end after the signal."""
    rng = np.random.default_rng(3)
    w, hop, pad, nframes, nE = 64, 17, 5, 9, 40
    x = rng.standard_normal(100)
    lo, xlo, df = erb_tables(w, nE, 1)
    window = np.hanning(w)
    mld = R.loudness(x, w, hop, pad, nframes, window, FS, lo, xlo, df, LD)
    bar = R.bar(np.abs(R.loudness(x, w, hop, pad, nframes, window, FS, lo, xlo, df) - mld).max())
    err = float(np.abs(gpu_loudness(x, w, hop, pad, nframes, window, lo, xlo, df) - mld).max())
    print("loudness uneven hop: error / bar %.3g" % (err / bar))
    assert err <= bar


# ---- 2. scores
def gpu_scores(K, L, nE):
    torch, c, d = ctx()
    cand, nframes = len(K), len(L)
    Si = torch.full((cand + 1, nframes), np.nan, dtype=torch.float64, device=d)
    c.swipe_scores(up(K), cand, K.shape[1], up(L), nframes, L.shape[1], nE, Si[:cand])
    out = Si.cpu().numpy()
    assert np.isnan(out[cand:]).all()
    return out[:cand]


@pytest.mark.parametrize("cand", (1, 16, 17, 192))
def test_scores_direct(amd, cand):
    """Every (nE, nframes) of the issue's lists: NaN in the unused columns of K and L, a zero last row of K and zero rows of
    L give exact zeros."""
    rng = np.random.default_rng(cand)
    worst = 0.0
    for nE in (1, 4, 5, 318, 427):
        for nframes in (1, 63, 64, 65, 130):
            K = np.full((cand, nE + 3), np.nan)
            L = np.full((nframes, nE + 1), np.nan)
            K[:, :nE] = rng.standard_normal((cand, nE)) / np.sqrt(nE)
            L[:, :nE] = np.abs(rng.standard_normal((nframes, nE))) / np.sqrt(nE)
            K[-1, :nE] = 0.0 if cand > 1 else K[-1, :nE]
            L[::7, :nE] = 0.0
            got = gpu_scores(K, L, nE)
            k, l = K[:, :nE], L[:, :nE]
            want = R.scores(k, l, LD)
            bar = 2 * nE * R.U * (np.abs(k) @ np.abs(l).T)
            err = np.abs(got - want).astype(np.float64)
            assert (cand == 1 or not got[-1].any()) and not got[:, ::7].any()               # exact on the zeros
            assert np.all(err <= bar), (nE, nframes)
            worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
            assert np.array_equal(got, gpu_scores(K, L, nE))
    print("scores cand=%d: worst error / bar %.3g" % (cand, worst))
    record_measurement("swipe_scores_%d" % cand, err_over_bar=worst)


# ---- 3. pick
def gpu_pick(windows, t, npc, pc0, ntc, nftc, ptab, nf, want_S=True):
    """windows: (Si, j0, mu, tshift) host arrays.  -> (p, s, S or None)"""
    torch, c, d = ctx()
    T = len(t)
    wins = [(up(Si), j0, len(mu), Si.shape[1], up(mu), up(ts)) for Si, j0, mu, ts in windows]
    p = torch.full((T + 4,), np.nan, dtype=torch.float64, device=d)
    s = torch.full((T + 4,), np.nan, dtype=torch.float64, device=d)
    S = torch.full((npc + 1, T), np.nan, dtype=torch.float64, device=d) if want_S else None
    c.swipe_pick(wins, up(t), T, npc, pc0, up(ntc), up(nftc), up(ptab), up(nf.astype(np.int32)), nftc.shape[1], p[:T], s[:T],
                 None if S is None else S[:npc])
    ph, sh = p.cpu().numpy(), s.cpu().numpy()
    assert np.isnan(ph[T:]).all() and np.isnan(sh[T:]).all()
    if S is None:
        return ph[:T], sh[:T], None
    Sh = S.cpu().numpy()
    assert np.isnan(Sh[npc:]).all()
    return ph[:T], sh[:T], Sh[:npc]


def check_pick(name, windows, t, npc, pc0, ntc, nftc, ptab, nf):
    m64 = R.pick(windows, t, npc, pc0, ntc, nftc, ptab, nf)
    mld = R.pick(windows, t, npc, pc0, ntc, nftc, ptab, nf, LD)
    p, s, S = gpu_pick(windows, t, npc, pc0, ntc, nftc, ptab, nf)
    p2, s2, none = gpu_pick(windows, t, npc, pc0, ntc, nftc, ptab, nf, want_S=False)
    assert none is None and np.array_equal(p, p2) and np.array_equal(s, s2)   # the same track without S
    dec = R.decided(mld, m64)
    bar_S = R.bar(np.abs(m64["S"] - mld["S"]).max())
    bar_s = R.bar(np.abs(m64["s"] - mld["s"]).max())
    eS, es = float(np.abs(S - mld["S"]).max()), float(np.abs(s - mld["s"])[dec].max()) if dec.any() else 0.0
    print("pick %s: %d of %d instants decided, S error / bar %.3g, s error / bar %.3g"
          % (name, dec.sum(), len(t), eS / bar_S, es / bar_s))
    record_measurement("swipe_pick_" + name, decided=int(dec.sum()), S_err_over_bar=eS / bar_S, s_err_over_bar=es / bar_s)
    assert np.array_equal(p[dec].view(np.uint64), mld["p"][dec].view(np.uint64))            # the pitch as bits
    assert eS <= bar_S and es <= bar_s
    assert np.all(np.isin(p, np.append(ptab.ravel(), pc0)))                  # every pitch comes from the table
    return p, s, S, mld, dec


def hand_tables(npc, nfine=16):
    """Symmetric abscissae, so that equal neighbours give an exactly even quadratic: c1 = 0 in the kernel's closed form."""
    ntc = np.tile(np.array([-0.125, 0.0, 0.125]), (npc, 1))
    nftc = np.tile((np.arange(nfine) - (nfine - 1) / 2) / 64.0, (npc, 1))    # +-1/128 are the two innermost points
    ptab = 100.0 + np.arange(npc)[:, None] + np.arange(nfine)[None, :] / 64.0
    nf = np.full(npc, nfine)
    ntc[[0, -1]] = 0
    nf[[0, -1]] = 0
    return ntc, nftc, ptab, nf


@pytest.mark.parametrize("T", (1, 63, 64, 65))
def test_pick_single_window(amd, T):
    """One window, mu = 1, frames exactly on the instants (t[-1] == tshift[-1]): S is the hand-made array up to the
    interpolation's rounding, and exactly so where a column repeats its left neighbour."""
    rng = np.random.default_rng(T)
    npc, nfr, pc0 = 70, max(T, 2), 99.0
    ts = np.arange(nfr) * 0.001
    t = ts[:T].copy()
    Si = rng.uniform(0.1, 1.0, (npc, nfr))
    plant = {}                                                               # instant -> (candidate, fine point) or None

    def column(m, values):                                                   # the column and its left neighbour alike
        Si[:, m] = values
        if m > 0:
            Si[:, m - 1] = values
    base = rng.uniform(0.1, 1.0, npc)
    first, last, inner, tie, zero, even = (base.copy() for _ in range(6))
    first[0] = 2.0
    column(0, first)
    plant[0] = None                                                          # candidate 0: p = pc0
    if T > 3:
        last[-1] = 2.0
        column(3, last)
        plant[3] = None                                                      # the last candidate: p = pc0 as well
        inner[20], inner[19], inner[21] = 2.0, 1.5, 1.75
        column(6, inner)
        tie[[5, 9]] = 2.0
        tie[[4, 6, 8, 10]] = 1.5
        column(9, tie)                                                       # two equal candidates: the first, 5
        zero[:] = 0.0
        column(12, zero)
        plant[12] = None
        even[30], even[29], even[31] = 2.0, 1.5, 1.5
        column(15, even)                                                     # an even quadratic: fine points 7 and 8 tie
    ntc, nftc, ptab, nf = hand_tables(npc)
    windows = [(Si, 0, np.ones(npc), ts)]
    p, s, S, mld, dec = check_pick("single_T%d" % T, windows, t, npc, pc0, ntc, nftc, ptab, nf)
    assert np.array_equal(S[:, 0], Si[:, 0])
    assert p[0] == pc0 and s[0] == 2.0
    if T > 3:
        for m in (3, 6, 9, 12, 15):
            assert np.array_equal(S[:, m], Si[:, m]), m                      # slope 0: the column itself
        assert p[3] == pc0 and s[3] == 2.0
        assert p[6] in ptab[20] and dec[6]
        assert p[9] in ptab[5] and not dec[9]                                # the tie goes to the first candidate
        assert p[12] == pc0 and s[12] == 0.0 and dec[12]
        assert p[15] == ptab[30, 7] and not dec[15]                          # ... and to the first fine point


@pytest.mark.parametrize("plim,count", (((160, 300), 2), ((100, 400), 3), ((70, 500), 4)))
def test_pick_overlapping_windows(amd, plim, count):
    """The plan's own windows (first / middle / last j, k, mu branches of swipe.py), random scores."""
    from eaqhm_amd import pitch
    plan = pitch.swipe_plan(1111, 16000, plim)
    assert len(plan["windows"]) == count
    rng = np.random.default_rng(count)
    windows = [(rng.uniform(0, 1, (w["ncand"], w["nframes"])), w["j0"], w["mu"], w["tshift"]) for w in plan["windows"]]
    for Si, _, _, _ in windows:
        Si[-1] = 0.0                                                         # the last candidate is never scored
    check_pick("plan_%d_windows" % count, windows, plan["t"], len(plan["pc"]), plan["pc"][0], plan["ntc"], plan["nftc"],
               plan["ptab"], plan["nf"])


# ---- 4. end to end
INPUTS = R.end_to_end_inputs()
_HOST = {}


def host(i):
    if i not in _HOST:
        from eaqhm_amd.swipe import swipep
        _, x, fs, plim = INPUTS[i]
        _HOST[i] = (swipep(x, fs, list(plim)), R.model(x, fs, plim), R.model(x, fs, plim, LD))
    return _HOST[i]


@pytest.mark.parametrize("i", range(4), ids=[c[0] for c in INPUTS])
def test_end_to_end_against_swipep(amd, i):
    from eaqhm_amd import pitch
    name, x, fs, plim = INPUTS[i]
    ref, m64, mld = host(i)
    got = pitch.swipep_device(x, fs, plim)
    again, S = pitch.swipep_device(x, fs, plim, return_strengths=True)
    dec = R.decided(mld, m64)
    bar_s = R.bar(np.abs(m64["s"] - mld["s"]).max())
    bar_S = R.bar(np.abs(m64["S"] - mld["S"]).max())
    es, eS = float(np.abs(got[:, 2] - ref[:, 2]).max()), float(np.abs(S - mld["S"]).max())
    print("%s: %d of %d instants decided, %d pitches differ from swipep, strength error / bar %.3g, S error / bar %.3g"
          % (name, dec.sum(), len(dec), (got[:, 1] != ref[:, 1]).sum(), es / bar_s, eS / bar_S))
    record_measurement("swipe_end_to_end_" + name, decided=int(dec.sum()), instants=len(dec),
                       pitch_differs=int((got[:, 1] != ref[:, 1]).sum()), s_err_over_bar=es / bar_s, S_err_over_bar=eS / bar_S)
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.array_equal(got[:, 0].view(np.uint64), ref[:, 0].view(np.uint64))
    assert dec.all()                                                         # the inputs leave nothing undecided
    assert np.array_equal(got[dec, 1].view(np.uint64), ref[dec, 1].view(np.uint64))
    assert es <= bar_s and eS <= bar_S
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))        # a second call, and the S path: the same bits
    assert S.shape == (len(mld["plan"]["pc"]), len(ref))
    if name == "sa19":
        g = load_golden("sa19_female_default.npz")["swipe_track"]
        assert got.shape == g.shape and np.abs(got[:, 0] - g[:, 0]).max() == 0
        assert np.abs(got[:, 1] - g[:, 1]).max() < 1e-9 and np.abs(got[:, 2] - g[:, 2]).max() < 1e-12


def test_digital_silence(amd):
    from eaqhm_amd import pitch
    from eaqhm_amd.swipe import swipep
    from eaqhm_amd.synth import synth_speech_int16
    x = synth_speech_int16(1.0, 16000) / 32768.0
    x[5600:10400] = 0.0                                                      # 0.3 s
    ref = swipep(x, 16000, [160, 300])
    mld = R.model(x, 16000, (160, 300), LD)
    got = pitch.swipep_device(x, 16000, (160, 300))
    quiet = ~np.asarray(mld["S"] != 0).any(axis=0)
    print("silence: %d quiet instants" % quiet.sum())
    assert quiet.sum() > 150 and np.all(ref[quiet, 1] == mld["plan"]["pc"][0]) and not ref[quiet, 2].any()
    assert np.array_equal(got[quiet].view(np.uint64), ref[quiet].view(np.uint64))
    dec = R.decided(mld)
    print("silence: %d quiet instants, %d of %d decided" % (quiet.sum(), dec.sum(), len(dec)))
    assert dec.sum() >= 0.99 * len(dec)
    assert np.array_equal(got[dec, 1].view(np.uint64), ref[dec, 1].view(np.uint64))
    assert np.abs(got[:, 2] - ref[:, 2])[dec].max() <= R.bar(np.abs(R.model(x, 16000, (160, 300))["s"] - mld["s"]).max())


# ---- 5. the analysis
def test_analysis_from_the_device_track(amd):
    from eaqhm_amd import pitch
    wav = os.path.join(GOLDEN, "SA19.WAV")
    ref = host(0)[0]
    track = pitch.analysis_pitch_track(wav, "female")
    assert track.shape == ref.shape and np.array_equal(track[:, 1].view(np.uint64), ref[:, 1].view(np.uint64))
    kw = dict(maxAdpt=1, printPrompts=False, loadingScreen=False)
    srer_dev = amd.eaQHMAnalysisAndSynthesis(wav, "female", pitch_track=track, **kw)[1]
    srer_host = amd.eaQHMAnalysisAndSynthesis(wav, "female", pitch_track=ref, **kw)[1]
    assert len(srer_dev) == len(srer_host) >= 2
    assert np.array_equal(np.asarray(srer_dev, dtype=np.float64).view(np.uint64),
                          np.asarray(srer_host, dtype=np.float64).view(np.uint64))


# ---- 6. bad arguments
def test_entry_points_refuse_bad_arguments(amd):
    """EAQHM_EINVAL (-1), nothing launched, the outputs untouched."""
    torch, c, d = ctx()
    lib, h = c.lib, c.h
    z = lambda n, dt=torch.float64: torch.zeros(n, dtype=dt, device=d)  # noqa: E731
    out = torch.full((64,), 7.0, dtype=torch.float64, device=d)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    x, win, lo, xlo, df = z(16), z(8), z(4, torch.int32), z(4), z(4)

    def loud(x=x, n=16, w=8, hop=4, pad=4, nframes=3, win=win, fs=16000.0, sw=1.0, lo=lo, xlo=xlo, df=df, nE=4, L=out, ld=4):
        return lib.eaqhm_swipe_loudness(h, P(x), n, w, hop, pad, nframes, P(win), fs, sw, P(lo), P(xlo), P(df), nE, P(L), ld)
    for bad in (dict(x=None), dict(win=None), dict(lo=None), dict(xlo=None), dict(df=None), dict(L=None), dict(n=0),
                dict(w=4), dict(w=12), dict(w=16384), dict(hop=0), dict(hop=9), dict(pad=-1), dict(nframes=0), dict(nE=0),
                dict(nE=1025), dict(ld=3), dict(fs=0.0), dict(sw=0.0)):
        assert loud(**bad) == -1, bad
    K, L = z(8), z(8)

    def score(K=K, cand=2, ldk=4, L=L, nframes=2, ldl=4, nE=4, Si=out):
        return lib.eaqhm_swipe_scores(h, P(K), cand, ldk, P(L), nframes, ldl, nE, P(Si))
    for bad in (dict(K=None), dict(L=None), dict(Si=None), dict(cand=0), dict(cand=4097), dict(nE=0), dict(nframes=0),
                dict(ldk=3), dict(ldl=3)):
        assert score(**bad) == -1, bad
    import ctypes as C
    Si, mu, ts, t, tab, nf = z(8), z(4), z(2), z(3), z(64), z(4, torch.int32)

    def pick(nwin=1, Si=Si, j0=0, ncand=4, nfr=2, mu=mu, ts=ts, t=t, T=3, npc=4, ntc=tab, nftc=tab, ptab=tab, nf=nf, nfmax=16,
             p=out, s=out[32:], arrays=True):
        if not arrays:
            return lib.eaqhm_swipe_pick(h, nwin, None, None, None, None, None, None, P(t), T, npc, 1.0, P(ntc), P(nftc),
                                        P(ptab), P(nf), nfmax, P(p), P(s), None)
        return lib.eaqhm_swipe_pick(h, nwin, (C.c_void_p * 1)(P(Si)), (C.c_int32 * 1)(j0), (C.c_int32 * 1)(ncand),
                                    (C.c_int64 * 1)(nfr), (C.c_void_p * 1)(P(mu)), (C.c_void_p * 1)(P(ts)), P(t), T, npc,
                                    1.0, P(ntc), P(nftc), P(ptab), P(nf), nfmax, P(p), P(s), None)
    for bad in (dict(arrays=False), dict(nwin=0), dict(nwin=9), dict(Si=None), dict(mu=None), dict(ts=None), dict(t=None),
                dict(T=0), dict(npc=2), dict(ntc=None), dict(nftc=None), dict(ptab=None), dict(nf=None), dict(nfmax=0),
                dict(nfmax=65), dict(p=None), dict(s=None), dict(nfr=1), dict(ncand=0), dict(j0=-1), dict(j0=1)):
        assert pick(**bad) == -1, bad
    c.sync()
    assert torch.all(out == 7.0).item()
    assert loud() == 0 and score() == 0 and pick() == 0                       # the same calls with good arguments run
    c.sync()
