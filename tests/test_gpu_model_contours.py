"""Time and pitch scale contours on the MI355X (model.eaQHMSynthesis with array scales -> eaqhm_modify_prep with gain,
eaqhm_modify_synth with the contour map): constant contours against the scalar path, agreement with the NumPy model of DESIGN.md §9.1
(tests/model_contour_ref.py), pitch and duration, locality, split ranges, additivity over slots and the CLI."""
import os

import numpy as np
import pytest
from scipy.io import wavfile

import model_contour_ref as MC
import model_synthesis_ref as M
from conftest import GOLDEN, load_golden, record_measurement
from test_gpu_model_synthesis import analyse, f0_law, reference_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


@pytest.fixture(scope="module")
def synth16k_fresh(amd, tmp_path_factory):
    from eaqhm_amd.synth import synth_speech_int16
    return analyse(amd, tmp_path_factory.mktemp("c16"), synth_speech_int16(2.0, 16000), 16000, "synth16k_2s")


@pytest.fixture(scope="module")
def synth48k_fresh(amd, tmp_path_factory):
    from eaqhm_amd.synth import synth_speech_int16
    return analyse(amd, tmp_path_factory.mktemp("c48"), synth_speech_int16(0.6, 48000), 48000, "synth48k_0p6s",
                   maxAdpt=1)


def contour_settings(n):
    """(label, rho, beta, preserve_envelope) per instant for a model of n instants."""
    i = np.arange(n)
    x = i / max(n - 1, 1)
    sinus = 1.1 + 0.5 * np.sin(2 * np.pi * 3.0 * x)                      # 0.6 .. 1.6
    ramp = 0.8 + 0.5 * x                                                 # 0.8 -> 1.3
    step = np.where((i // 20) % 2 == 0, 0.5, 2.0)
    limits = np.where((i // 15) % 3 == 0, 0.25, np.where((i // 15) % 3 == 1, 4.0, 1.0))
    one = np.ones(n)
    return [("rho_sinus", sinus, one, True),
            ("beta_ramp", one, ramp, True),
            ("both_noenv", sinus, 1.3 - 0.5 * x, False),
            ("rho_step", step, one, True),
            ("limits", limits, limits[::-1].copy(), True)]


def test_constant_contours_equal_scalar_path(amd, synth16k_fresh):
    g, det = reference_model()
    s_recon, _, arrays = synth16k_fresh
    for label, d, ref0 in (("sa19", det, g["s_recon"]), ("synth16k", arrays, s_recon)):
        n, L = len(d["ti"]), len(ref0)
        out = amd.eaQHMSynthesis(d, 16000, L, time_scale=np.ones(n), pitch_scale=np.ones(n))
        err = float(np.abs(out - ref0).max())
        record_measurement("model_contours_unit_vs_s_recon_%s" % label, max_abs=err)
        assert out.shape == ref0.shape and err <= 1e-9, (label, err)
        for rho in (0.75, 1.5, 2.0):
            for beta in (1.0, 1.2):
                ref = amd.eaQHMSynthesis(d, 16000, L, time_scale=rho, pitch_scale=beta)
                out = amd.eaQHMSynthesis(d, 16000, L, time_scale=np.full(n, rho), pitch_scale=np.full(n, beta))
                rel = float(np.abs(out - ref).max() / np.abs(ref).max())
                assert out.shape == ref.shape and rel <= 1e-9, (label, rho, beta, rel)


def _gpu_vs_numpy(amd, det, fs, L, label, bar=1e-8, settings=None):
    from eaqhm_amd.model import unpack_model
    m = unpack_model(det)
    n = len(m["records"])
    worst = 0.0
    for name, rho, beta, env in (settings or contour_settings(n)):
        out = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, preserve_envelope=env)
        ref = MC.synthesize_contour(m["records"], m["step"], fs, L, rho, beta, env)
        assert out.shape == ref.shape == (MC.time_map(rho, beta, m["step"], L)[3],)
        rel = float(np.abs(out - ref).max() / np.abs(ref).max())
        record_measurement("model_contours_vs_numpy_%s_%s" % (label, name), max_rel=rel)
        worst = max(worst, rel)
        assert rel <= bar, (name, rel)
    return worst


def test_gpu_against_numpy_contour_model_sa19(amd):
    g, det = reference_model()
    _gpu_vs_numpy(amd, det, 16000, len(g["s_recon"]), "sa19")


def test_gpu_against_numpy_contour_model_synth16k(amd, synth16k_fresh):
    s_recon, _, arrays = synth16k_fresh
    _gpu_vs_numpy(amd, arrays, 16000, len(s_recon), "synth16k_2s")


def test_gpu_against_numpy_contour_model_48k(amd, synth48k_fresh):
    """Large Kmax, short runs (kind-3 pieces) and isolated knots at 48 kHz."""
    from eaqhm_amd.model import unpack_model
    s_recon, _, arrays = synth48k_fresh
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


def test_60s_model_against_numpy_contour_model(amd, tmp_path):
    """synth16k_60s (one analysis run): the bar is 1e-7 of the maximum for the reason test_gpu_model_synthesis gives
    (unwrapped phases of ~1e6 rad summed in a different order on the GPU and in NumPy)."""
    from eaqhm_amd.model import unpack_model
    from eaqhm_amd.synth import synth_speech_int16
    grid = np.load(os.path.join(GOLDEN, "prep_fixtures.npz"))["synth16k_60s_f0s_5ms"]
    s_recon, _, arrays = analyse(amd, tmp_path, synth_speech_int16(60.0, 16000), 16000, "synth16k_60s", maxAdpt=5,
                                 track=grid)
    n = len(arrays["ti"])
    t = np.arange(n) * 15 / 16000.0
    rho = 1.05 + 0.35 * np.sin(2 * np.pi * 0.5 * t)
    beta = np.interp(t, [0.0, t[-1]], [0.85, 1.2])
    _gpu_vs_numpy(amd, arrays, 16000, len(s_recon), "synth16k_60s", bar=1e-7,
                  settings=[("both", rho, beta, True)])


def test_pitch_and_duration(amd, synth16k_fresh):
    """SWIPE' on the output follows b(tau(t')) * f0_law(tau(t')) and the length is L_out."""
    from eaqhm_amd.model import contour_time_map
    from eaqhm_amd.swipe import swipep
    s_recon, structs, _ = synth16k_fresh
    L, fs, D = len(s_recon), 16000, 15
    n = len(structs)
    t = np.arange(n) * D / fs
    rho = 1.15 + 0.3 * np.sin(2 * np.pi * 0.4 * t)
    beta = 1.1 + 0.15 * np.sin(2 * np.pi * 0.3 * t + 1.0)
    out = amd.eaQHMSynthesis(structs, fs, L, time_scale=rho, pitch_scale=beta)
    tm = contour_time_map(rho, beta, D, L)
    assert len(out) == tm["L_out"]
    tr = swipep(out, fs, [120, 500])
    tp, f = tr[:, 0], tr[:, 1]
    j, r = MC.locate(tm["C"], tm["rate"], D, len(out))
    idx = np.clip(np.rint(tp * fs).astype(np.int64), 0, len(out) - 1)
    jj, tau = j[idx], (j[idx] * D + r[idx]) / fs
    b = (beta[np.minimum(jj, n - 2)] + beta[np.minimum(jj + 1, n - 1)]) / 2
    want = b * f0_law(tau)
    sel = (tau >= 0.2) & (tau <= 1.8) & np.isfinite(f)
    assert sel.sum() > 0.9 * np.count_nonzero((tau >= 0.2) & (tau <= 1.8))
    rel = np.abs(f[sel] - want[sel]) / want[sel]
    med, p95 = float(np.median(rel)), float(np.percentile(rel, 95))
    record_measurement("model_contours_pitch", median_rel=med, p95_rel=p95)
    assert med <= 0.01 and p95 <= 0.03


def test_locality_and_split_ranges(amd, synth16k_fresh):
    """Changing the contours from instant m on leaves out[:floor(C_{m-1})] bit-identical; [0, L/2) and [L/2, L)
    computed separately are bit-for-bit the whole output."""
    from eaqhm_amd.model import contour_time_map
    s_recon, _, arrays = synth16k_fresh
    L, n = len(s_recon), len(arrays["ti"])
    x = np.arange(n) / (n - 1)
    rho = 0.9 + 0.4 * x
    beta = 1.2 - 0.3 * x
    m = n // 2
    rho2, beta2 = rho.copy(), beta.copy()
    rho2[m:] = 0.3
    beta2[m:] = 1.7
    a = amd.eaQHMSynthesis(arrays, 16000, L, time_scale=rho, pitch_scale=beta)
    b = amd.eaQHMSynthesis(arrays, 16000, L, time_scale=rho2, pitch_scale=beta2)
    cut = int(np.floor(contour_time_map(rho, beta, 15, L)["C"][m - 1]))
    assert cut > 1000 and np.array_equal(a[:cut], b[:cut])
    assert not np.array_equal(a[cut + 200:cut + 400], b[cut + 200:cut + 400])
    h = len(a) // 2
    split = amd.eaQHMSynthesis(arrays, 16000, L, time_scale=rho, pitch_scale=beta, _ranges=[(0, h), (h, len(a))])
    assert np.array_equal(split, a)


def test_contours_are_additive_over_slots(amd, synth16k_fresh):
    s_recon, _, arrays = synth16k_fresh
    L = len(s_recon)
    K = arrays["amplitudes"].shape[1]
    n = len(arrays["ti"])
    x = np.arange(n) / (n - 1)
    rho, beta = 0.8 + 0.7 * x, 1.3 - 0.4 * x

    def keep(slots):
        d = dict(arrays)
        am = np.zeros_like(arrays["amplitudes"])
        am[:, slots] = arrays["amplitudes"][:, slots]
        d["amplitudes"] = am
        return amd.eaQHMSynthesis(d, 16000, L, time_scale=rho, pitch_scale=beta, preserve_envelope=False)

    A, B = list(range(0, K, 2)), list(range(1, K, 2))
    s_all, s_a, s_b, s_0 = keep(A + B), keep(A), keep(B), keep([])
    scale = np.abs(s_all).max()
    assert np.abs((s_all - s_0) - ((s_a - s_0) + (s_b - s_0))).max() <= 1e-12 * scale


def test_cli_curves_write_modified_wav(amd, tmp_path):
    import shutil
    from eaqhm_amd import cli
    from eaqhm_amd.model import contour_time_map, scale_contour
    wav = str(tmp_path / "SA19.WAV")
    shutil.copy(os.path.join(GOLDEN, "SA19.WAV"), wav)
    tc, pc = tmp_path / "time.txt", tmp_path / "pitch.txt"
    tc.write_text("# seconds  time scale\n0.5 1.0\n1.5 1.6\n3.0 0.8\n")
    pc.write_text("# seconds  pitch scale\n0.0 0.9\n\n3.9 1.2\n")
    assert cli.main([wav, "--gender", "female", "--max-adpt", "1", "--time-scale-curve", str(tc),
                     "--pitch-scale-curve", str(pc)]) == 0
    fs, y = wavfile.read(str(tmp_path / "SA19_modified.wav"))
    det = dict(ti=load_golden("sa19_female_default.npz")["det_ti"])
    rho = scale_contour(det, 16000, [0.5, 1.5, 3.0], [1.0, 1.6, 0.8])
    beta = scale_contour(det, 16000, [0.0, 3.9], [0.9, 1.2])
    assert fs == 16000 and y.dtype == np.float32
    assert y.shape == (contour_time_map(rho, beta, 15, 63488)["L_out"],)
    assert np.all(np.isfinite(y)) and np.abs(y).max() > 0.01
    for flags in (["--time-scale", "1.2", "--time-scale-curve", str(tc)],
                  ["--pitch-scale", "1.2", "--pitch-scale-curve", str(pc)]):
        with pytest.raises(SystemExit):
            cli.main([wav] + flags)
