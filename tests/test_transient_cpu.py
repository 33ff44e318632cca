"""Transient onsets without a GPU: the NumPy model of tests/transient_ref.py against the conditions the
definition was chosen under (a synthetic signal with four bursts, silence, a constant, SA19), the host side of
eaqhm_amd.transient (plan, whole frames, the wait rule, the protection weight, the protected time scale), every argument
check, the CLI flags with stand-ins, the plumbing, and five deliberate errors in the model that the bars must see."""
import inspect
import os
import re

import numpy as np
import pytest

import transient_ref as R
from conftest import ROOT, load_golden

PKG = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd")
LD = np.longdouble


@pytest.fixture(scope="module")
def T():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import transient
    return transient


@pytest.fixture(scope="module")
def bursts(T):
    """fs -> (x, burst times, the model in float64, in long double)."""
    out = {}
    for fs in (16000, 48000):
        x, times = R.burst_signal(fs)
        out[fs] = (x, times, R.model(x, fs), R.model(x, fs, LD))
    return out


@pytest.fixture(scope="module")
def sa19(T):
    """(model of SA19, the analysed model's instants as an arrays model, length)."""
    x, fs = R.sa19()
    g = load_golden("sa19_female_default.npz")
    assert fs == 16000 and len(g["s_recon"]) == len(x)
    return R.model(x, fs), dict(ti=g["det_ti"]), len(x)


# ---- 1. the conditions the definition was chosen under
@pytest.mark.parametrize("fs", [16000, 48000])
def test_four_bursts(bursts, fs):
    x, times, m, mld = bursts[fs]
    hop, nf = m["hop"], len(m["d"])
    assert hop == round(0.005 * fs) and m["window"] == {16000: 256, 48000: 512}[fs] and nf == (len(x) - 1) // hop + 1
    print("fs %d: onsets at frames %s, d %s" % (fs, m["frames"].tolist(), np.round(m["d"][m["frames"]], 3).tolist()))
    assert len(m["frames"]) == 4
    assert np.abs(m["frames"] - times * fs / hop).max() <= 1                 # each within one frame of its burst
    if fs == 16000:
        assert m["d"][m["frames"]].min() >= 3.1                              # the bursts of amplitude 0.1 included
    lo, hi = m["whole"]
    assert lo >= 1 and hi < nf - 1                                           # a cut-off frame on either side
    assert not m["d"][:lo + 2].any() and not m["d"][hi + 1:].any()           # exact zeros: m < lag, or not whole
    assert not m["flag"][:10].any() and not m["flag"][-10:].any()
    assert np.array_equal(m["frames"], mld["frames"])


@pytest.mark.parametrize("x", [np.zeros(16000), np.full(16000, 0.5)], ids=["zeros", "constant"])
def test_degenerate_signals(T, x):
    m = R.model(x, 16000)
    assert not m["d"].any() and not m["flag"].any() and len(m["frames"]) == 0
    inner = m["L"][m["whole"][0]:m["whole"][1] + 1]
    assert (inner == inner[0]).all()                                         # whole frames of a constant: equal rows


def test_sa19_onsets_and_contour(T, sa19):
    """On the plateaus the interval rate is exactly 1 and every knot is the float64 sum C[j] + step.  Read back as a
    difference, C[j + 1] - C[j] is exactly `step` wherever both knots lie in one binade; where C passes a power of two
    (1024, 4096, 8192 samples: five plateau intervals over the four scales) the knot's last bit is rounded and the
    difference is off by 1.1e-13 to 9.1e-13, whatever the contour, so those intervals are checked in the forward form
    alone."""
    from eaqhm_amd.records import contour_time_map
    m, det, length = sa19
    fs, step = 16000, int(det["ti"][1])
    K = len(m["frames"])
    p = T.protection_weight(det, fs, m["times"])
    print("SA19: %d onsets at frames %s, protected share %.4f" % (K, m["frames"].tolist(), p.mean()))
    assert 12 <= K <= 32
    assert p.min() >= 0 and p.max() == 1 and p.mean() < 0.4
    both = (p[:-1] == 1) & (p[1:] == 1)
    assert both.sum() > 100
    lows, highs = [], []
    for rho in (0.5, 1.5, 2, 3):
        r, info = T.protect_time_scale(det, fs, length, rho, m["times"], return_info=True)
        plain = contour_time_map(np.full(len(r), float(rho)), np.ones(len(r)), step, length)["L_out"]
        tm = contour_time_map(r, np.ones(len(r)), step, length)
        lows.append(r.min())
        highs.append(r.max())
        assert info["clipped"] == 0 and info["c"] > 0
        assert info["L_out"] == tm["L_out"] and abs(tm["L_out"] - plain) <= 1
        assert np.all(r[p == 1] == 1.0)
        C = tm["C"]                                                          # the plateaus run at rate exactly 1
        assert np.all(tm["rate"][:-1][both] == 1.0) and np.all(C[1:][both] == C[:-1][both] + step)
        binade = np.frexp(C[:-1])[1] == np.frexp(C[1:])[1]
        assert np.all(np.diff(C)[both & binade] == step) and (~binade).sum() <= 18                 # one a power of two
        assert np.array_equal(r, T.protect_time_scale(det, fs, length, np.full(len(r), float(rho)), m["times"]))
    print("SA19: protected contours between %.4g and %.4g" % (min(lows), max(highs)))
    assert min(lows) >= 0.25 and max(highs) <= 4.0


def test_clip_and_nothing_left(T, sa19):
    m, det, length = sa19
    with pytest.raises(ValueError, match="nothing is left"):                 # a third of the file at rate 1 is longer
        T.protect_time_scale(det, 16000, length, 0.25, m["times"])           # than a quarter of the file: c <= 0
    for rho, times in ((0.25, m["times"][:3]), (0.4, m["times"])):          # 0 < c < 1 pushes the rest below the range:
        r, info = T.protect_time_scale(det, 16000, length, rho, times, return_info=True)   # clipped, not an error
        assert 0 < info["c"] < 1 and info["clipped"] > 0 and r.min() == 0.25 and r.max() == 1.0
    everywhere = np.arange(0, length / 16000.0, 0.04)                        # plateaus of 50 ms every 40 ms: p = 1
    assert np.all(T.protection_weight(det, 16000, everywhere) == 1)
    with pytest.raises(ValueError, match="nothing is left"):
        T.protect_time_scale(det, 16000, length, 2.0, everywhere)
    with pytest.raises(ValueError, match="nothing is left"):                 # c <= 0: the plateaus alone are too long
        T.protect_time_scale(det, 16000, length, 0.3, np.arange(0, length / 16000.0, 0.075))
    r = T.protect_time_scale(det, 16000, length, 2.0, [])                    # no onsets: the scale as it was
    assert np.all(r == 2.0)


# ---- 2. the host side
def test_onset_plan_edges(T):
    for fs, w in ((16000, 256), (48000, 512)):
        win, k = T.onset_plan(fs)
        assert len(win) == w and k.dtype == np.int32 and len(k) == 25
        assert np.all(np.diff(k) > 0) and k[-1] == w // 2 + 1 and k[0] == int(np.ceil(100.0 * w / fs))
        i = np.arange(w)
        assert np.array_equal(win, 0.5 - 0.5 * np.cos(2 * np.pi * (i + 0.5) / w))
        assert np.allclose(win, win[::-1], rtol=0, atol=4 * R.U) and 0 < win.min() and win.max() < 1
    win, k = T.onset_plan(16000, 32, 1, 0.0)
    assert k.tolist() == [0, 17]
    _, k = T.onset_plan(16000, 64, 32, 0.0)                                  # more bands than the ERB spacing separates
    assert np.all(np.diff(k) >= 1) and k[-1] == 33 and (np.diff(k) == 1).sum() > 10
    _, k = T.onset_plan(8000, 2048, 64, 50.0)
    assert np.all(np.diff(k) > 0) and k[-1] == 1025
    with pytest.raises(ValueError, match="no band may be empty"):
        T.onset_plan(16000, 32, 24, 100.0)
    assert T.onset_plan(16000, 64, 33, 0.0)[1].tolist() == list(range(34))   # a bin a band
    with pytest.raises(ValueError, match="no band may be empty"):
        T.onset_plan(16000, 64, 34, 0.0)


def test_whole_frames_and_wait(T):
    for n, hop, w in ((1000, 80, 256), (100, 1, 32), (31, 8, 32), (32, 8, 32), (33, 48, 32), (5000, 4096, 2048), (16, 4, 32)):
        nf = (n - 1) // hop + 1
        whole = [m for m in range(nf + 2) if m * hop - w // 2 >= 0 and m * hop + w // 2 - 1 <= n - 1]
        lo, hi = T.whole_frames(n, hop, w)
        assert list(range(lo, hi + 1)) == whole, (n, hop, w)
        assert hi < nf
    assert T.keep_onsets([3, 12, 13, 14, 24, 25, 40], 10).tolist() == [3, 14, 25, 40]
    assert T.keep_onsets([3, 4, 5], 0).tolist() == [3, 4, 5]
    assert T.keep_onsets([], 10).tolist() == [] and T.keep_onsets([], 10).dtype == np.int64


def test_protection_weight_shape(T):
    det = dict(ti=np.arange(0, 16000, 16))                                   # an instant every millisecond
    p = T.protection_weight(det, 16000, [0.5])
    t = det["ti"] / 16000.0
    assert np.all(p[(t >= 0.49) & (t <= 0.54)] == 1) and not p[(t <= 0.48 - 1e-9) | (t >= 0.55 + 1e-9)].any()
    up = (t > 0.48) & (t < 0.49)
    assert np.allclose(p[up], (t[up] - 0.48) / 0.01, rtol=0, atol=1e-12)
    down = (t > 0.54) & (t < 0.55)
    assert np.allclose(p[down], (0.55 - t[down]) / 0.01, rtol=0, atol=1e-12)
    two = T.protection_weight(det, 16000, [0.5, 0.56])
    assert np.array_equal(two, np.maximum(p, T.protection_weight(det, 16000, [0.56])))
    box = T.protection_weight(det, 16000, [0.5], before=0.0, after=0.002, ramp=0.0)
    assert set(np.unique(box)) == {0.0, 1.0} and box.sum() == 3
    assert not T.protection_weight(det, 16000, []).any()
    structs = [type("Det", (), dict(ti=int(v)))() for v in det["ti"][:40]]
    assert np.array_equal(T.protection_weight(structs, 16000, [0.01]), T.protection_weight(dict(ti=det["ti"][:40]), 16000,
                                                                                           [0.01]))


def test_contour_length_is_what_the_time_map_rounds(T):
    from eaqhm_amd.records import contour_time_map
    rng = np.random.default_rng(5)
    r = rng.uniform(0.25, 4, 300)
    for step, length in ((15, 299 * 15 + 1), (80, 299 * 80 + 57)):
        assert int(np.rint(T.contour_length(r, step, length))) == contour_time_map(r, np.ones(300), step, length)["L_out"]
    a, b = rng.uniform(0, 1, 300), rng.uniform(0, 1, 300)
    assert abs(T.contour_length(a + 2 * b, 15, 5000) - T.contour_length(a, 15, 5000) - 2 * T.contour_length(b, 15, 5000)) < 1e-8


# ---- 3. every argument check
def test_argument_checks(T):
    x = np.zeros(4000)
    bad = [dict(s=np.zeros((2, 5))), dict(s=[]), dict(s=[0.0, np.nan]), dict(s=[0.0, np.inf]), dict(s=np.zeros(4, complex)),
           dict(s=["a", "b"]), dict(fs=0), dict(fs=-16000), dict(fs=np.nan), dict(fs="x"), dict(window=100), dict(window=16),
           dict(window=4096), dict(window=256.5), dict(hop=0), dict(hop=4097), dict(hop=2.5), dict(bands=0), dict(bands=65),
           dict(bands=24, window=32), dict(fmin=-1), dict(fmin=8000), dict(fmin=np.nan), dict(lag=0), dict(lag=17),
           dict(floor=0), dict(floor=-1e-9), dict(floor=np.inf)]
    for kw in bad:
        args = dict(s=x, fs=16000)
        args.update(kw)
        with pytest.raises(ValueError):
            T.check_onset_arguments(**args)
        with pytest.raises(ValueError):                                      # before any device work
            T.onset_strength(args.pop("s"), args.pop("fs"), **args)
    xs, fs, hop, win, k, lag, floor = T.check_onset_arguments(list(range(200)), 8000)
    assert xs.dtype == np.float64 and (fs, hop, len(win), len(k), lag, floor) == (8000.0, 40, 128, 25, 2, 1e-9)
    with pytest.raises(ValueError):
        T.onset_strength(x, 16000, device_index=-1)
    od = dict(d=np.zeros(5), hop=80, fs=16000)
    for kw in (dict(delta=-0.1), dict(delta=np.nan), dict(pre_max=-1), dict(post_max=65), dict(pre_avg=1.5),
               dict(post_avg=65), dict(wait=-1), dict(wait=2.5), dict(device_index=True)):
        with pytest.raises(ValueError):
            T.onsets(od, **kw)
    for broken in ([0.0, 1.0], dict(d=np.zeros(5)), dict(d=np.zeros((2, 2)), hop=80, fs=16000), dict(d=[], hop=80, fs=16000),
                   dict(d=[0.0, -1.0], hop=80, fs=16000), dict(d=[0.0, np.nan], hop=80, fs=16000),
                   dict(d=np.zeros(5), hop=0, fs=16000), dict(d=np.zeros(5), hop=80, fs=0)):
        with pytest.raises(ValueError):
            T.onsets(broken)
    assert T.check_peak_arguments() == (0.5, 3, 3, 20, 6, 10)
    det = dict(ti=np.arange(0, 1600, 16))
    for kw in (dict(times=[-0.1]), dict(times=[np.nan]), dict(times=[[0.1]]), dict(times=["a"]), dict(before=-1e-3),
               dict(after=-1e-3), dict(ramp=-1e-3), dict(ramp=np.inf), dict(fs=0)):
        args = dict(fs=16000, times=[0.05])
        args.update(kw)
        fs, times = args.pop("fs"), args.pop("times")
        with pytest.raises(ValueError):
            T.protection_weight(det, fs, times, **args)
        with pytest.raises(ValueError):
            T.protect_time_scale(det, fs, 1600, 2.0, times, **args)
    for model in (dict(ti=[0]), dict(ti=[0, 16, 40]), dict(ti=[16, 32, 48]), None, dict(tj=[0, 16])):
        with pytest.raises(ValueError):
            T.protection_weight(model, 16000, [0.05])
    for scale in (np.full(99, 2.0), np.full(101, 2.0), 5.0, 0.1, np.full(100, 5.0), "x"):   # a contour of the wrong length
        with pytest.raises(ValueError):
            T.protect_time_scale(det, 16000, 1600, scale, [0.05])
    with pytest.raises(ValueError):
        T.protect_time_scale(det, 16000, 1000, 2.0, [0.05])                  # shorter than the model


# ---- 4. the model against itself, and the five deliberate errors
def test_model_precisions_agree(bursts, sa19):
    cases = [("burst16k",) + bursts[16000][2:], ("burst48k",) + bursts[48000][2:]]
    x, fs = R.sa19()
    cases.append(("sa19", sa19[0], R.model(x, fs, LD)))
    for name, m, mld in cases:
        dd = float(np.abs(m["d"] - mld["d"]).max())
        dL = float(np.abs(m["L"] - mld["L"]).max())
        bar_d = R.bar(dd, np.abs(mld["d"]).max())
        dec = R.decided(m, mld, bar_d)
        print("%s: |d64 - dld| %.2e, |L64 - Lld| %.2e, bar on d %.2e, decided %d of %d"
              % (name, dd, dL, bar_d, dec.sum(), len(dec)))
        assert dd < 1e-12 and dL < 1e-11
        assert dec.mean() > 0.99 and np.array_equal(m["flag"][dec], mld["flag"][dec])
        assert np.array_equal(R.flux(m["L"], 2, *m["whole"]), m["d"])


def test_deliberate_errors_are_seen(bursts):
    x, _, m, mld = bursts[16000]
    bar_L = R.bar(np.abs(m["L"] - mld["L"]).max(), np.abs(mld["L"]).max())
    bar_d = R.bar(np.abs(m["d"] - mld["d"]).max(), np.abs(mld["d"]).max())
    assert np.abs(m["L"] - mld["L"]).max() <= bar_L and np.abs(m["d"] - mld["d"]).max() <= bar_d
    for fault in ("window_half", "kB_short"):                                # seen in the band energies
        f = R.model(x, 16000, fault=fault)
        assert np.abs(f["L"] - mld["L"]).max() > bar_L, fault
    for fault in ("lag_minus", "no_whole"):                                  # the bands are right, the flux is not
        f = R.model(x, 16000, fault=fault)
        assert np.array_equal(f["L"], m["L"]) and np.abs(f["d"] - mld["d"]).max() > bar_d, fault
    f = R.model(x, 16000, fault="no_whole")
    assert f["d"][-1] > 1 and f["frames"][-1] == len(f["d"]) - 1             # the file's end read as an onset
    d = np.zeros(40)
    d[[10, 11, 12]] = 2.0                                                    # a plateau: the first frame is the onset
    right, wrong = R.peaks(d), R.peaks(d, ties_last=True)
    assert np.flatnonzero(right).tolist() == [10] and np.flatnonzero(wrong).tolist() == [12]


def test_peaks_by_hand():
    d = np.array([0.0, 3.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 2.0])
    assert np.flatnonzero(R.peaks(d, 1, 1, 1, 1, 0.5)).tolist() == [1, 4, 8]
    assert np.flatnonzero(R.peaks(d, 3, 3, 1, 1, 0.5)).tolist() == [1, 8]   # 4 lies in the window of 1
    assert np.flatnonzero(R.peaks(d, 1, 1, 8, 8, 0.5)).tolist() == [1, 8]   # mean 2/3: 1.0 < 2/3 + 0.5
    assert np.flatnonzero(R.peaks(d, 0, 0, 0, 0, 0.0)).tolist() == [1, 4, 8]   # d >= d
    assert not R.peaks(d, 0, 0, 0, 0, 0.1).any()
    assert not R.peaks(np.zeros(5), 0, 0, 0, 0, 0.0).any()                  # d > 0
    assert R.peaks(np.array([2.0]), 64, 64, 64, 64, 0.0).tolist() == [1]


# ---- 5. plumbing
def test_symbols_header_and_makefile(T):
    from eaqhm_amd import hip
    counts = dict(eaqhm_onset_bands=13, eaqhm_onset_flux=9, eaqhm_onset_peaks=9)
    assert hip.ABI_VERSION == 6
    bound = {name: len(args) for name, _, args in hip.SYMBOLS_ONSET}
    others = (hip.SYMBOLS + hip.SYMBOLS_MLPG + hip.SYMBOLS_GV + hip.SYMBOLS_CEPWARP + hip.SYMBOLS_KMEANS
              + hip.SYMBOLS_MLPG_EM + hip.SYMBOLS_NN + hip.SYMBOLS_SWIPE + hip.SYMBOLS_VITERBI + hip.SYMBOLS_FORMANT)
    assert not set(bound) & {name for name, _, _ in others}
    header = open(os.path.join(ROOT, "include", "eaqhm_onset.h")).read()
    assert '#include "eaqhm_onset.h"' in open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t)\s+(eaqhm_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(bound) == set(counts)
    for name, n in counts.items():
        assert bound[name] == n, name
        decl = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, header, re.M)
        assert decl is not None and len(decl.group(1).split(",")) == n, name
    assert "DESIGN.md §15" in header
    for name in ("onset_bands", "onset_flux", "onset_peaks"):
        assert callable(getattr(hip.Context, name))
    for const, macro in ((T.ONSET_WINDOW_RANGE[0], "EAQHM_ONSET_WMIN"), (T.ONSET_WINDOW_RANGE[1], "EAQHM_ONSET_WMAX"),
                         (T.ONSET_HOP_MAX, "EAQHM_ONSET_HOP"), (T.ONSET_BANDS_MAX, "EAQHM_ONSET_BANDS"),
                         (T.ONSET_LAG_MAX, "EAQHM_ONSET_LAG"), (T.ONSET_SPAN_MAX, "EAQHM_ONSET_SPAN")):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, header).group(1)) == const
    lib = hip.load_library()                                                 # a null context: EAQHM_EINVAL
    assert lib.eaqhm_onset_bands(None, None, 1, 32, 1, 1, None, 1.0, None, 1, 1e-9, None, 1) == -1
    assert lib.eaqhm_onset_flux(None, None, 1, 1, 1, 1, 0, 0, None) == -1
    assert lib.eaqhm_onset_peaks(None, None, 1, 0, 0, 0, 0, 0.5, None) == -1
    makefile = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\beaqhm_onset\.hip\b", makefile, re.M)
    assert re.search(r"^HDR\s*:=.*include/eaqhm_onset\.h\b", makefile, re.M)
    source = open(os.path.join(PKG, "csrc", "eaqhm_onset.hip")).read()
    assert "#pragma clang fp contract(off)" in source and "atomic" not in source.replace("No atomics", "")


def test_not_reexported_and_surface_unchanged(T):
    import json
    import eaqhm_amd
    for name in ("onset_strength", "onsets", "protection_weight", "protect_time_scale", "onset_plan"):
        assert callable(getattr(T, name)) and not hasattr(eaqhm_amd, name)
    assert "§15" in T.__doc__
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "python_api.json")))["eaqhm_amd"]
    assert {n for n in vars(eaqhm_amd) if not n.startswith("_") and not inspect.ismodule(getattr(eaqhm_amd, n))
            and getattr(getattr(eaqhm_amd, n), "__module__", "eaqhm_amd").startswith("eaqhm_amd")} <= set(recorded)
    assert str(inspect.signature(T.onset_strength)) == \
        ("(s, fs, *, hop=None, window=None, bands=24, fmin=100.0, lag=2, floor=1e-09, return_bands=False, "
         "device_index=0)")
    assert str(inspect.signature(T.onsets)) == \
        "(od, *, delta=0.5, pre_max=3, post_max=3, pre_avg=20, post_avg=6, wait=10, device_index=0)"
    assert str(inspect.signature(T.protection_weight)) == \
        "(DetComponents, fs, times, *, before=0.01, after=0.04, ramp=0.01)"
    assert str(inspect.signature(T.protect_time_scale)) == \
        "(DetComponents, fs, length, time_scale, times, *, before=0.01, after=0.04, ramp=0.01, return_info=False)"
    assert str(inspect.signature(T.onset_plan)) == "(fs, window=None, bands=24, fmin=100.0)"


def test_cli_flags(T, monkeypatch, tmp_path, capsys):
    from eaqhm_amd import cli
    a = cli.parser().parse_args(["x.wav"])
    assert a.protect_transients is False and a.transient_delta is None and a.onsets_out is None
    for flag in ("--protect-transients", "--transient-delta", "--onsets-out"):
        assert flag in cli.__doc__
    for argv in (["x.wav", "--protect-transients"], ["x.wav", "--protect-transients", "--pitch-scale", "1.2"],
                 ["x.wav", "--transient-delta", "0.4"], ["x.wav", "--onsets-out", "o.txt", "--transient-delta", "-1"],
                 ["x.wav", "--protect-transients", "--time-scale", "2", "--transient-delta", "nan"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
    capsys.readouterr()
    # stand-ins: the analysis, the detector and the synthesis
    from scipy.io import wavfile
    from eaqhm_amd import model
    wav = str(tmp_path / "a.wav")
    wavfile.write(wav, 16000, np.zeros(16000, np.int16))
    det = dict(ti=np.arange(0, 16000, 80))
    calls, synth = [], []
    monkeypatch.setattr(cli, "analyse", lambda path, gender, opts: (np.zeros(16000), [0.0], det, None))
    monkeypatch.setattr(cli, "onset_table", lambda path, fc, delta=None:
                        calls.append((os.path.basename(path), fc, delta)) or (np.array([0.25, 0.6]), np.array([3.0, 1.5])))
    monkeypatch.setattr(model, "eaQHMSynthesis", lambda d, fs, L, **kw: synth.append(kw) or np.zeros(L))
    out = str(tmp_path / "onsets.txt")
    assert cli.main([wav, "--onsets-out", out, "--transient-delta", "0.4"]) == 0
    assert calls == [("a.wav", 0, 0.4)] and synth == []
    assert np.array_equal(np.loadtxt(out), [[0.25, 3.0], [0.6, 1.5]])
    assert open(out).readline().split() == ["#", "seconds", "strength"]
    del calls[:]
    assert cli.main([wav, "--time-scale", "2", "--protect-transients", "--phase", "shape"]) == 0
    assert calls == [("a.wav", 0, None)]
    rho = synth[0]["time_scale"]
    want, info = T.protect_time_scale(det, 16000, 16000, 2.0, [0.25, 0.6], return_info=True)
    assert np.array_equal(rho, want) and synth[0]["phase"] == "shape" and rho.min() == 1.0 and rho.max() > 2.0
    assert "protected 2 transients" in capsys.readouterr().out
    assert os.path.exists(wav[:-4] + "_modified.wav")
    curve = str(tmp_path / "curve.txt")
    np.savetxt(curve, [[0.0, 1.0], [1.0, 3.0]])
    del synth[:], calls[:]
    assert cli.main([wav, "--time-scale-curve", curve, "--protect-transients", "--onsets-out", out]) == 0
    assert len(calls) == 1 and len(synth[0]["time_scale"]) == len(det["ti"])
    assert np.all(synth[0]["time_scale"][T.protection_weight(det, 16000, [0.25, 0.6]) == 1] == 1.0)
    del synth[:], calls[:]
    assert cli.main([wav, "--time-scale", "2"]) == 0                         # without the flags: the call as it was
    assert calls == [] and synth[0]["time_scale"] == 2.0
