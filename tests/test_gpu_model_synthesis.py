"""Resynthesis from the model on the MI355X (model.eaQHMSynthesis -> eaqhm_modify_prep / eaqhm_modify_synth): the
identity with the analysis's s_recon, agreement with the NumPy model of the definition (tests/model_synthesis_ref.py),
the pitch and duration of the result, additivity over slots, a 60 s model and the CLI."""
import os

import numpy as np
import pytest
from scipy.interpolate import make_interp_spline
from scipy.io import wavfile

import model_synthesis_ref as M
from conftest import GOLDEN, load_golden, record_measurement

pytestmark = pytest.mark.gpu

SETTINGS = [(1.5, 1.0, True), (0.7, 1.0, True), (1.0, 1.3, True), (1.0, 0.8, True), (1.25, 0.9, False),
            (0.5, 2.0, True)]


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


def f0_law(t):
    """The pitch of synth.synth_speech (closed form)."""
    return 220.0 + 40.0 * np.sin(2 * np.pi * 0.31 * t) + 10.0 * np.sin(2 * np.pi * 1.7 * t)


def analyse(amd, tmp_dir, x_int16, fs, name, maxAdpt=10, track=None):
    """Fresh GPU analysis of an int16 signal: (s_recon, structs model, arrays model)."""
    from eaqhm_amd.functions import pack_arrays, pack_results
    path = os.path.join(str(tmp_dir), name + ".wav")
    wavfile.write(path, fs, x_int16)
    if track is None:
        t = np.arange(0, len(x_int16) / fs, 0.001)
        track = np.column_stack([t, f0_law(t)])
    s_recon, _, _, _, eng = amd.eaQHMAnalysisAndSynthesis(path, "female", maxAdpt=maxAdpt, printPrompts=False,
                                                          pitch_track=track, _return_engine=True)
    fin = eng.final_arrays()
    return s_recon, pack_results(eng.plan, fin), pack_arrays(eng.plan, fin)


@pytest.fixture(scope="module")
def sa19_fresh(amd, tmp_path_factory):
    g = load_golden("sa19_female_default.npz")
    fs, x = wavfile.read(os.path.join(GOLDEN, "SA19.WAV"))
    return analyse(amd, tmp_path_factory.mktemp("sa19"), x, fs, "SA19", track=g["swipe_track"])


@pytest.fixture(scope="module")
def synth16k_fresh(amd, tmp_path_factory):
    from eaqhm_amd.synth import synth_speech_int16
    return analyse(amd, tmp_path_factory.mktemp("s16"), synth_speech_int16(2.0, 16000), 16000, "synth16k_2s")


@pytest.fixture(scope="module")
def synth48k_fresh(amd, tmp_path_factory):
    from eaqhm_amd.synth import synth_speech_int16
    return analyse(amd, tmp_path_factory.mktemp("s48"), synth_speech_int16(0.6, 48000), 48000, "synth48k_0p6s",
                   maxAdpt=1)


def reference_model():
    """The model the reference itself returned for SA19 (det_* arrays of the fixture) in the arrays form."""
    g = load_golden("sa19_female_default.npz")
    cells = g["det_cells"]
    n = len(g["det_ti"])
    K = int(cells[:, 1].max()) + 1
    i, k = cells[:, 0], cells[:, 1]
    d = dict(ti=g["det_ti"], isVoiced=g["det_isVoiced"], a0=np.where(g["det_isVoiced"], g["det_a0"], 0.0))
    for name, key in (("amplitudes", "det_am"), ("frange", "det_fm"), ("pk", "det_pk")):
        a = np.zeros((n, K))
        a[i, k] = g[key]
        d[name] = a
    return g, d


def test_identity_reference_model(amd):
    g, det = reference_model()
    out = amd.eaQHMSynthesis(det, 16000, len(g["s_recon"]))
    err = float(np.abs(out - g["s_recon"]).max())
    record_measurement("model_synthesis_identity_reference_sa19", max_abs=err)
    assert out.dtype == np.float64 and out.shape == g["s_recon"].shape
    assert err <= 1e-9


@pytest.mark.parametrize("which", ["sa19", "synth16k"])
def test_identity_fresh_analysis(which, request):
    amd = request.getfixturevalue("amd")
    s_recon, structs, arrays = request.getfixturevalue(which + "_fresh")
    fs = 16000
    for form, det in (("structs", structs), ("arrays", arrays)):
        out = amd.eaQHMSynthesis(det, fs, len(s_recon))
        err = float(np.abs(out - s_recon).max())
        record_measurement("model_synthesis_identity_%s_%s" % (which, form), max_abs=err)
        assert out.shape == s_recon.shape and err <= 1e-9, (form, err)


def _gpu_vs_numpy(amd, det, fs, L, label):
    from eaqhm_amd.model import unpack_model
    m = unpack_model(det)
    worst = 0.0
    for rho, beta, env in SETTINGS:
        out = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, preserve_envelope=env)
        ref = M.synthesize(m["records"], m["step"], fs, L, rho, beta, env)
        assert out.shape == ref.shape == (int(np.rint(rho * L)),)
        rel = float(np.abs(out - ref).max() / np.abs(ref).max())
        record_measurement("model_synthesis_vs_numpy_%s_rho%g_beta%g_env%d" % (label, rho, beta, env), max_rel=rel)
        worst = max(worst, rel)
        assert rel <= 1e-8, (rho, beta, env, rel)
    return worst


def test_gpu_against_numpy_model_sa19(amd):
    g, det = reference_model()
    _gpu_vs_numpy(amd, det, 16000, len(g["s_recon"]), "sa19")


def test_gpu_against_numpy_model_synth16k(amd, synth16k_fresh):
    s_recon, _, arrays = synth16k_fresh
    _gpu_vs_numpy(amd, arrays, 16000, len(s_recon), "synth16k_2s")


def test_gpu_against_numpy_model_48k(amd, synth48k_fresh):
    """Large Kmax and short runs (kind-3 pieces) at 48 kHz."""
    from eaqhm_amd.model import unpack_model
    s_recon, _, arrays = synth48k_fresh
    # an edited copy: slots 3..14 cut into runs of 3, 2 and 1 knots (kind-3 pieces, isolated knots)
    d = dict(arrays)
    am = arrays["amplitudes"].copy()
    i = np.arange(am.shape[0])[:, None]
    for lo, period in ((3, 4), (7, 3), (11, 2)):
        cols = slice(lo, lo + 4)
        am[:, cols] = np.where(i % period == 0, 0.0, am[:, cols])
    d["amplitudes"] = am
    rec = unpack_model(d)["records"]
    K = (rec.shape[1] - 1) // 3
    code, _ = M.run_codes(rec[:, :K] != 0)
    assert K > 100 and np.any(code >= 16) and np.any(code == 1)
    _gpu_vs_numpy(amd, arrays, 48000, len(s_recon), "synth48k_0p6s")
    _gpu_vs_numpy(amd, d, 48000, len(s_recon), "synth48k_0p6s_short_runs")


@pytest.mark.parametrize("rho, beta", [(1.5, 1.25), (1.5, 1.0)])
def test_pitch_and_duration(amd, synth16k_fresh, rho, beta):
    """2 s of synthetic female speech whose f0 law is known: the output is rho times as long and SWIPE' finds beta times
    the law at t'/rho."""
    from eaqhm_amd.swipe import swipep
    s_recon, structs, _ = synth16k_fresh
    L = len(s_recon)
    out = amd.eaQHMSynthesis(structs, 16000, L, time_scale=rho, pitch_scale=beta)
    assert len(out) == int(np.rint(rho * L))
    tr = swipep(out, 16000, [120, 500])
    t, f = tr[:, 0], tr[:, 1]
    tau = t / rho
    sel = (tau >= 0.2) & (tau <= 1.8) & np.isfinite(f)
    assert sel.sum() > 0.9 * np.count_nonzero((tau >= 0.2) & (tau <= 1.8))
    rel = np.abs(f[sel] - beta * f0_law(tau[sel])) / (beta * f0_law(tau[sel]))
    med, p95 = float(np.median(rel)), float(np.percentile(rel, 95))
    record_measurement("model_synthesis_pitch_rho%g_beta%g" % (rho, beta), median_rel=med, p95_rel=p95)
    assert med <= 0.01 and p95 <= 0.03


def test_edited_models_are_additive_over_slots(amd, synth16k_fresh):
    """Without the envelope every slot is synthesised on its own: synth(A u B) - synth(0) = the sum of the parts, and
    the model with every slot zeroed is the a0 spline."""
    s_recon, _, arrays = synth16k_fresh
    L = len(s_recon)
    K = arrays["amplitudes"].shape[1]

    def keep(slots):
        d = dict(arrays)
        am = np.zeros_like(arrays["amplitudes"])
        am[:, slots] = arrays["amplitudes"][:, slots]
        d["amplitudes"] = am
        return amd.eaQHMSynthesis(d, 16000, L, time_scale=1.3, pitch_scale=1.2, preserve_envelope=False)

    A, B = list(range(0, K, 2)), list(range(1, K, 2))
    s_all, s_a, s_b, s_0 = keep(A + B), keep(A), keep(B), keep([])
    scale = np.abs(s_all).max()
    assert np.abs((s_all - s_0) - ((s_a - s_0) + (s_b - s_0))).max() <= 1e-12 * scale
    n = len(arrays["ti"])
    tau = np.arange(len(s_0)) / 1.3
    a0 = make_interp_spline(np.arange(n) * 15.0, arrays["a0"], k=3)(tau, extrapolate=True)
    assert np.abs(s_0 - a0).max() <= 1e-12 * max(np.abs(a0).max(), 1e-300)


def test_60s_model_against_numpy_model(amd, tmp_path):
    """synth16k_60s (one analysis run).  Runs span tens of thousands of knots here, so the unwrapped phases reach
    ~1e6 rad and their rounding (a parallel scan on the GPU, a sequential sum in NumPy) is ~1e-10 rad: the bar is 1e-7
    of the signal's maximum instead of 1e-8."""
    from eaqhm_amd.model import unpack_model
    from eaqhm_amd.synth import synth_speech_int16
    grid = np.load(os.path.join(GOLDEN, "prep_fixtures.npz"))["synth16k_60s_f0s_5ms"]
    s_recon, _, arrays = analyse(amd, tmp_path, synth_speech_int16(60.0, 16000), 16000, "synth16k_60s", maxAdpt=5,
                                 track=grid)
    L = len(s_recon)
    out = amd.eaQHMSynthesis(arrays, 16000, L, time_scale=2.0, pitch_scale=1.1)
    m = unpack_model(arrays)
    ref = M.synthesize(m["records"], m["step"], 16000, L, 2.0, 1.1, True)
    rel = float(np.abs(out - ref).max() / np.abs(ref).max())
    record_measurement("model_synthesis_60s_vs_numpy", max_rel=rel)
    assert out.shape == ref.shape and rel <= 1e-7


def test_cli_writes_modified_wav(amd, tmp_path, capsys):
    import shutil
    from eaqhm_amd import cli
    wav = str(tmp_path / "SA19.WAV")
    shutil.copy(os.path.join(GOLDEN, "SA19.WAV"), wav)
    assert cli.main([wav, "--gender", "female", "--max-adpt", "1", "--time-scale", "1.2", "--pitch-scale", "0.9"]) == 0
    fs, x = wavfile.read(str(tmp_path / "SA19_reconstructed.wav"))
    assert fs == 16000 and x.dtype == np.float32 and x.shape == (63488,)
    fs, y = wavfile.read(str(tmp_path / "SA19_modified.wav"))
    assert fs == 16000 and y.dtype == np.float32 and y.shape == (int(np.rint(1.2 * 63488)),)
    assert np.all(np.isfinite(y)) and np.abs(y).max() > 0.01
