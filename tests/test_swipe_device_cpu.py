"""The host side of the device SWIPE' (eaqhm_amd.pitch) and its model (tests/swipe_ref.py), without a GPU: the model is
swipe.swipep on the four end-to-end inputs of tests/test_gpu_swipe.py, those inputs leave no instant to a tie, the plan's
tables are swipe.py's, and the argument checks, the binding, the header and the CLI flag are what DESIGN.md §13 says."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import swipe_ref as R  # noqa: E402

PKG = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd")
INPUTS = R.end_to_end_inputs()
_CACHE = {}


def runs(i):
    """(swipep's track, the float64 model, the long-double model) of input i, computed once."""
    if i not in _CACHE:
        from eaqhm_amd.swipe import swipep
        _, x, fs, plim = INPUTS[i]
        _CACHE[i] = (swipep(x, fs, list(plim)), R.model(x, fs, plim), R.model(x, fs, plim, np.longdouble))
    return _CACHE[i]


@pytest.mark.parametrize("i", range(4), ids=[c[0] for c in INPUTS])
def test_model_is_swipep(i):
    ref, m, ml = runs(i)
    assert m["track"].shape == ref.shape and np.array_equal(m["track"][:, 0], ref[:, 0])
    assert np.array_equal(m["track"][:, 1], ref[:, 1])                       # the pitch bit for bit
    ds = np.abs(m["track"][:, 2] - ref[:, 2]).max() / R.U
    print("%s: strength within %.1f u of swipep" % (INPUTS[i][0], ds))
    assert ds <= 16
    assert np.array_equal(m["p"], ml["p"]) and np.array_equal(m["i"], ml["i"]) and np.array_equal(m["k"], ml["k"])
    print("%s: float64 vs long double: |dS| %.2e, |ds| %.2e" % (INPUTS[i][0], float(np.abs(m["S"] - ml["S"]).max()),
                                                                 float(np.abs(m["s"] - ml["s"]).max())))


@pytest.mark.parametrize("i", range(4), ids=[c[0] for c in INPUTS])
def test_inputs_leave_few_instants_undecided(i):
    """A condition on the inputs, not a measurement of any code under test."""
    _, m, ml = runs(i)
    dec = R.decided(ml, m)
    print("%s: %d of %d instants undecided, least gaps %.2e / %.2e"
          % (INPUTS[i][0], (~dec).sum(), len(dec), ml["gap1"].min(), ml["gap2"].min()))
    assert (~dec).sum() <= 0.01 * len(dec)


def test_window_sizes_of_the_inputs():
    got = [[w["w"] for w in runs(i)[1]["plan"]["windows"]] for i in range(4)]
    assert got[1] == [2048, 1024, 512, 256] and got[3][0] == 4096 and got[0] == [1024, 512]


@pytest.mark.parametrize("i", range(4), ids=[c[0] for c in INPUTS])
def test_plan_kernel_rows_are_strength_ones(i):
    from eaqhm_amd.swipe import _strength_one
    plan = runs(i)[1]["plan"]
    f = plan["fERBs"]
    eye = np.eye(len(f))
    covered = np.zeros(len(plan["pc"]), dtype=int)
    for w in plan["windows"]:
        K, j = w["K"], w["j"]
        assert K.shape == (len(j), len(f)) and np.array_equal(j, np.arange(w["j0"], w["j0"] + w["ncand"]))
        assert not K[-1].any()                                               # the last candidate is never scored
        for r in range(len(j) - 1):
            ref = _strength_one(f, eye, plan["pc"][j[r]])
            assert np.abs(K[r] - ref).max() <= 2 * R.U * np.abs(ref).max(), (w["w"], r)
        covered[j] += 1
    assert covered.min() >= 1 and covered.max() <= 2                         # at most two windows per candidate


@pytest.mark.parametrize("i", range(4), ids=[c[0] for c in INPUTS])
def test_ptab_holds_swipeps_pitches(i):
    ref, m, _ = runs(i)
    plan = m["plan"]
    table = set(plan["ptab"][1:-1].ravel().view(np.uint64).tolist()) | {np.float64(plan["pc"][0]).view(np.uint64).item()}
    assert set(ref[:, 1].view(np.uint64).tolist()) <= table
    inner = np.flatnonzero(m["k"] >= 0)
    assert np.array_equal(plan["ptab"][m["i"][inner], m["k"][inner]], ref[inner, 1])
    assert plan["nf"][0] == 0 and plan["nf"][-1] == 0 and plan["nf"][1:-1].min() >= 1


def test_plan_geometry_and_cache():
    from eaqhm_amd import pitch
    plan = pitch.swipe_plan(16000, 16000, (160, 300))
    assert pitch.swipe_plan(16000, 16000.0, [160, 300]) is plan              # cached on (n, fs, tuple(plim))
    assert pitch.swipe_plan(16001, 16000, (160, 300))["windows"][0]["K"] is plan["windows"][0]["K"]   # K on (fs, plim)
    assert np.array_equal(plan["t"], np.arange(0, 1.0, 0.001))
    for w in plan["windows"]:
        assert w["hop"] == w["w"] // 2 and w["pad"] == w["w"] // 2 and w["nframes"] == len(w["tshift"])
        assert np.array_equal(w["window"], np.hanning(w["w"])) and w["lo"].dtype == np.int32
        assert w["lo"].min() >= 0 and w["lo"].max() <= w["w"] // 2 - 1 and (w["df"] > 0).all() and (w["xlo"] >= 0).all()
        assert (w["nframes"] - 1) * w["hop"] - w["pad"] < 16000              # the last frame still touches the signal


CASES = (
    (dict(x=np.zeros((4, 4))), "1-D"), (dict(x=np.zeros(0)), "empty"), (dict(x=np.array([0.0, np.nan, 1.0])), "finite"),
    (dict(x=np.array([0.0, np.inf])), "finite"), (dict(x=np.array(["a", "b"])), "numbers"), (dict(fs=0), "fs"),
    (dict(fs=-16000), "fs"), (dict(fs=np.nan), "fs"), (dict(plim=(160,)), "plim"), (dict(plim=(160, 300, 400)), "plim"),
    (dict(plim=(300, 160)), "plim"), (dict(plim=(0, 300)), "plim"), (dict(plim=(160, np.inf)), "plim"),
    (dict(plim=(160, 8001)), "plim"), (dict(plim=(160, 161)), "candidates"), (dict(plim=(10, 300)), "8192"),
    (dict(fs=96000, plim=(60, 500)), "8192"),
)


@pytest.mark.parametrize("change,match", CASES, ids=[str(n) for n in range(len(CASES))])
def test_check_swipe_arguments(change, match, monkeypatch):
    from eaqhm_amd import pitch
    monkeypatch.setattr(pitch, "_device_plan", lambda *a: pytest.fail("device work before the checks"))
    args = dict(x=np.zeros(800), fs=16000, plim=(160, 300))
    args.update(change)
    for fn in (pitch.check_swipe_arguments, pitch.swipep_device):
        with pytest.raises(ValueError, match=match):
            fn(**args)


def test_check_swipe_arguments_accepts_and_names_the_fitting_limit():
    from eaqhm_amd import pitch
    x, fs, plim = pitch.check_swipe_arguments([0, 1, 2, 3, 4], 16000, [160, 300])
    assert x.dtype == np.float64 and x.shape == (5,) and fs == 16000.0 and plim == (160.0, 300.0)
    with pytest.raises(ValueError) as e:
        pitch.check_swipe_arguments(np.zeros(100), 16000, (10, 300))
    fit = float(re.search(r"plim\[0\] above ([0-9.]+) Hz", str(e.value)).group(1))
    assert "8192" in str(e.value) and 11.04 < fit < 11.06                    # 8 fs / 2^13.5
    pitch.check_swipe_arguments(np.zeros(100), 16000, (fit * 1.001, 300))
    with pytest.raises(ValueError, match="8192"):
        pitch.check_swipe_arguments(np.zeros(100), 16000, (fit * 0.999, 300))
    # swipep's own refusal, the same words (no signal reaches it with swipep's frame geometry: the frames outlast t)
    ts = np.array([0.0, 0.016, 0.032])
    pitch._check_time_range(np.array([0.0, 0.032]), ts)
    for t in (np.array([0.0, 0.033]), np.array([-0.001, 0.03])):
        with pytest.raises(ValueError, match="A value in x_new is outside the interpolation range."):
            pitch._check_time_range(t, ts)


def test_symbols_header_and_makefile():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import hip
    counts = dict(eaqhm_swipe_loudness=16, eaqhm_swipe_scores=9, eaqhm_swipe_pick=20)
    assert hip.ABI_VERSION == 6
    bound = {name: len(args) for name, _, args in hip.SYMBOLS_SWIPE}
    others = (hip.SYMBOLS + hip.SYMBOLS_MLPG + hip.SYMBOLS_GV + hip.SYMBOLS_CEPWARP + hip.SYMBOLS_KMEANS
              + hip.SYMBOLS_MLPG_EM + hip.SYMBOLS_NN)
    assert not set(bound) & {name for name, _, _ in others}
    header = open(os.path.join(ROOT, "include", "eaqhm_swipe.h")).read()
    assert '#include "eaqhm_swipe.h"' in open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t)\s+(eaqhm_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(bound) == set(counts)
    for name, n in counts.items():
        assert bound[name] == n, name
        decl = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, header, re.M)
        assert decl is not None and len(decl.group(1).split(",")) == n, name
    for name in ("swipe_loudness", "swipe_scores", "swipe_pick"):
        assert callable(getattr(hip.Context, name))
    from eaqhm_amd import pitch
    for const, macro in (("SWIPE_WINDOW_MAX", "EAQHM_SWIPE_WMAX"), ("SWIPE_ERB_MAX", "EAQHM_SWIPE_EMAX"),
                         ("SWIPE_WINDOWS_MAX", "EAQHM_SWIPE_WINDOWS"), ("SWIPE_FINE_MAX", "EAQHM_SWIPE_FINE")):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, header).group(1)) == getattr(pitch, const)
    lib = hip.load_library()                                                 # a null context: EAQHM_EINVAL
    assert lib.eaqhm_swipe_loudness(None, None, 1, 8, 4, 4, 1, None, 1.0, 1.0, None, None, None, 1, None, 1) == -1
    assert lib.eaqhm_swipe_scores(None, None, 1, 1, None, 1, 1, 1, None) == -1
    assert lib.eaqhm_swipe_pick(None, 1, None, None, None, None, None, None, None, 1, 3, 1.0, None, None, None, None, 1,
                                None, None, None) == -1
    makefile = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\beaqhm_swipe\.hip\b", makefile, re.M)
    assert re.search(r"^HDR\s*:=.*include/eaqhm_swipe\.h\b", makefile, re.M)


def test_not_reexported_and_surface_unchanged():
    import eaqhm_amd
    from eaqhm_amd import pitch
    for name in ("swipep_device", "swipe_plan", "analysis_pitch_track", "check_swipe_arguments"):
        assert callable(getattr(pitch, name)) and not hasattr(eaqhm_amd, name)
    assert "§13" in pitch.__doc__
    import json
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "python_api.json")))["eaqhm_amd"]
    assert str(inspect.signature(eaqhm_amd.eaQHMAnalysisAndSynthesis)) == recorded["eaQHMAnalysisAndSynthesis"]["signature"]
    assert "pitch_track=None" in recorded["eaQHMAnalysisAndSynthesis"]["signature"]
    assert {n for n in vars(eaqhm_amd) if not n.startswith("_") and not inspect.ismodule(getattr(eaqhm_amd, n))
            and getattr(getattr(eaqhm_amd, n), "__module__", "eaqhm_amd").startswith("eaqhm_amd")} <= set(recorded)
    assert str(inspect.signature(pitch.swipep_device)) == "(x, fs, plim, *, device_index=0, return_strengths=False)"
    assert str(inspect.signature(pitch.analysis_pitch_track)) == "(speechFile, gender, fc=0, *, device_index=0)"


def test_prepare_still_calls_the_host_tracker(monkeypatch):
    """_prepare's default is swipe.swipep: the device tracker is used only where a track is handed over."""
    from eaqhm_amd import functions, pitch, swipe
    called = []
    monkeypatch.setattr(swipe, "swipep", lambda s, fs, plim: called.append((fs, plim)))
    monkeypatch.setattr(pitch, "swipep_device", lambda *a, **k: pytest.fail("the device tracker ran by default"))

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop
    monkeypatch.setattr(functions.prologue, "resample_track", stop)
    with pytest.raises(Stop):
        functions._prepare(os.path.join(ROOT, "tests", "golden", "SA19.WAV"), "female", 15, 1, 3, 32, True, 0, 0, None, 0)
    assert called == [(16000, [160, 300])]


def test_cli_flag(monkeypatch):
    from eaqhm_amd import cli, pitch
    assert cli.parser().parse_args(["x.wav"]).pitch_device is False
    assert cli.parser().parse_args(["x.wav", "--pitch-device"]).pitch_device is True
    assert "--pitch-device" in cli.__doc__
    seen = []
    monkeypatch.setattr(cli, "eaQHMAnalysisAndSynthesis", lambda path, gender, **o: seen.append((path, o)) or "result")
    monkeypatch.setattr(pitch, "analysis_pitch_track", lambda path, gender, fc=0: ("track of", path, gender, fc))
    assert cli.analyse("a.wav", "male", dict(step=15, fc=3)) == "result"      # without the flag: the call as it was
    assert cli.analyse("b.wav", "male", dict(step=15, fc=3, pitch_device=True)) == "result"
    assert seen == [("a.wav", dict(step=15, fc=3)),
                    ("b.wav", dict(step=15, fc=3, pitch_track=("track of", "b.wav", "male", 3)))]
