"""The shape-invariant phase mode on the MI355X (model.eaQHMSynthesis with phase="shape" -> eaqhm_modify_synth with
f0 and S, on either time map): agreement with the NumPy model of DESIGN.md §11 (tests/model_shape_ref.py), unit
scales against the default mode and s_recon, a constructed model with a closed-form answer, locality, noise and the
CLI."""
import os

import numpy as np
import pytest
from scipy.io import wavfile

import model_shape_ref as MS
from conftest import GOLDEN, record_measurement
from test_gpu_model_synthesis import analyse, reference_model

pytestmark = pytest.mark.gpu

SCALES = [(2.0, 1.0), (0.5, 1.0), (1.0, 1.3), (1.6, 0.8)]


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


@pytest.fixture(scope="module")
def synth16k_fresh(amd, tmp_path_factory):
    from eaqhm_amd.synth import synth_speech_int16
    return analyse(amd, tmp_path_factory.mktemp("h16"), synth_speech_int16(2.0, 16000), 16000, "synth16k_2s")


@pytest.fixture(scope="module")
def synth48k_fresh(amd, tmp_path_factory):
    from eaqhm_amd.synth import synth_speech_int16
    return analyse(amd, tmp_path_factory.mktemp("h48"), synth_speech_int16(0.6, 48000), 48000, "synth48k_0p6s",
                   maxAdpt=1)


def shape_settings(n):
    """(label, rho, beta, preserve_envelope, alpha): the scalar settings, one contour pair, a formant scale and a
    setting without the envelope."""
    x = np.arange(n) / max(n - 1, 1)
    sinus = 1.1 + 0.5 * np.sin(2 * np.pi * 3.0 * x)
    ramp = 1.3 - 0.5 * x
    out = [("rho%g_beta%g" % (r, b), r, b, True, None) for r, b in SCALES]
    out += [("contours", sinus, ramp, True, None),
            ("formant", 1.25, 1.2, True, 0.85),
            ("formant_contour", sinus, 1.0, True, 0.8 + 0.4 * x),
            ("noenv", 1.5, 0.9, False, None),
            ("contours_noenv", sinus, ramp, False, None)]
    return out


def _gpu_vs_numpy(amd, det, fs, L, label, bar=1e-8, settings=None):
    from eaqhm_amd.model import unpack_model
    m = unpack_model(det)
    n = len(m["records"])
    for name, rho, beta, env, alpha in (settings or shape_settings(n)):
        kw = {} if alpha is None else dict(formant_scale=alpha)
        out = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, preserve_envelope=env, phase="shape",
                                 **kw)
        ref = MS.synthesize_shape(m["records"], m["step"], fs, L, rho, beta, env, alpha=alpha)
        assert out.shape == ref.shape
        rel = float(np.abs(out - ref).max() / np.abs(ref).max())
        record_measurement("model_shape_vs_numpy_%s_%s" % (label, name), max_rel=rel)
        print("shape vs numpy", label, name, rel)
        assert rel <= bar, (label, name, rel)


def test_gpu_against_numpy_shape_model_sa19(amd):
    g, det = reference_model()
    _gpu_vs_numpy(amd, det, 16000, len(g["s_recon"]), "sa19")


def test_gpu_against_numpy_shape_model_synth16k(amd, synth16k_fresh):
    s_recon, structs, arrays = synth16k_fresh
    _gpu_vs_numpy(amd, arrays, 16000, len(s_recon), "synth16k_2s")
    a = amd.eaQHMSynthesis(arrays, 16000, len(s_recon), time_scale=2.0, phase="shape")
    b = amd.eaQHMSynthesis(structs, 16000, len(s_recon), time_scale=2.0, phase="shape")
    a0 = amd.eaQHMSynthesis(arrays, 16000, len(s_recon), time_scale=2.0)
    b0 = amd.eaQHMSynthesis(structs, 16000, len(s_recon), time_scale=2.0)
    print("arrays vs structs: shape", float(np.abs(a - b).max()), "independent", float(np.abs(a0 - b0).max()),
          "f0", float(np.abs(amd.model_f0(arrays, 16000) - amd.model_f0(structs, 16000)).max()))
    # both det_formats hold the same model ("structs" drops trailing empty slots, which add exact zeros everywhere)
    assert np.array_equal(a, b)


def test_gpu_against_numpy_shape_model_48k(amd, synth48k_fresh):
    """Large Kmax, short runs (kind-3 pieces) and isolated knots at 48 kHz."""
    s_recon, _, arrays = synth48k_fresh
    d = dict(arrays)
    am = arrays["amplitudes"].copy()
    i = np.arange(am.shape[0])[:, None]
    for lo, period in ((3, 4), (7, 3), (11, 2)):
        cols = slice(lo, lo + 4)
        am[:, cols] = np.where(i % period == 0, 0.0, am[:, cols])
    d["amplitudes"] = am
    _gpu_vs_numpy(amd, arrays, 48000, len(s_recon), "synth48k_0p6s")
    _gpu_vs_numpy(amd, d, 48000, len(s_recon), "synth48k_0p6s_short_runs")


def test_60s_model_against_numpy_shape_model(amd, tmp_path):
    """synth16k_60s (one analysis run): the bar is 1e-7 of the maximum for the reason
    test_gpu_model_synthesis.test_60s_model_against_numpy_model gives (unwrapped phases of ~1e6 rad summed in a different
    order on the GPU and in NumPy)."""
    from eaqhm_amd.synth import synth_speech_int16
    grid = np.load(os.path.join(GOLDEN, "prep_fixtures.npz"))["synth16k_60s_f0s_5ms"]
    s_recon, _, arrays = analyse(amd, tmp_path, synth_speech_int16(60.0, 16000), 16000, "synth16k_60s", maxAdpt=5,
                                 track=grid)
    n = len(arrays["ti"])
    t = np.arange(n) * 15 / 16000.0
    rho = 1.05 + 0.35 * np.sin(2 * np.pi * 0.5 * t)
    beta = np.interp(t, [0.0, t[-1]], [0.85, 1.2])
    _gpu_vs_numpy(amd, arrays, 16000, len(s_recon), "synth16k_60s", bar=1e-7,
                  settings=[("rho2_beta1.1", 2.0, 1.1, True, None), ("both", rho, beta, True, None)])


def test_unit_scales_equal_default_mode_and_s_recon(amd, synth16k_fresh):
    """At g_j = 1 the advance s is exactly 0: the shape kernels add an exact zero and weigh by 1.0."""
    g, det = reference_model()
    s_recon, _, arrays = synth16k_fresh
    for label, d, ref0 in (("sa19", det, g["s_recon"]), ("synth16k", arrays, s_recon)):
        n, L = len(d["ti"]), len(ref0)
        for form, one in (("scalar", 1.0), ("contour", np.ones(n))):
            a = amd.eaQHMSynthesis(d, 16000, L, time_scale=one, pitch_scale=one, phase="shape")
            b = amd.eaQHMSynthesis(d, 16000, L, time_scale=one, pitch_scale=one)
            rel = float(np.abs(a - b).max() / np.abs(b).max())
            bits = bool(np.array_equal(a, b))
            err = float(np.abs(a - ref0).max())
            record_measurement("model_shape_unit_%s_%s" % (label, form), max_rel_vs_default=rel, bit_equal=bits,
                               max_abs_vs_s_recon=err)
            print("unit scales", label, form, "rel", rel, "bit equal", bits, "vs s_recon", err)
            assert rel <= 1e-12 and err <= 1e-9, (label, form, rel, err)


def test_constructed_model_keeps_its_shape(amd):
    """A model whose answer is known in closed form (model_shape_ref.constructed_model).  The bar is the distance of the
    NumPy model from the closed form, measured here (1.5e-7 of the maximum, DESIGN.md §11: the cubic interpolation of
    the tracks between knots), plus the 1e-8 the kernels are held to against the NumPy model."""
    det, L, closed = MS.constructed_model()
    from eaqhm_amd.model import unpack_model
    m = unpack_model(det)
    f0 = np.full(len(det["ti"]), 140.0)
    for rho, beta in SCALES:
        want, N = closed(rho, beta)
        top = np.abs(want).max()
        ref = MS.synthesize_shape(m["records"], 15, 16000, L, rho, beta, False, f0=f0)
        d_ref = float(np.abs(ref[:N] - want).max() / top)
        out = amd.eaQHMSynthesis(det, 16000, L, time_scale=rho, pitch_scale=beta, preserve_envelope=False,
                                 phase="shape", f0=f0)
        d_gpu = float(np.abs(out[:N] - want).max() / top)
        record_measurement("model_shape_closed_form_rho%g_beta%g" % (rho, beta), numpy=d_ref, gpu=d_gpu)
        print("closed form", rho, beta, "numpy", d_ref, "gpu", d_gpu)
        assert d_ref <= 1e-6                          # the NumPy model itself follows the closed form
        assert d_gpu <= d_ref + 1e-8, (rho, beta, d_gpu, d_ref)
    want, N = closed(2.0, 1.0)
    ind = amd.eaQHMSynthesis(det, 16000, L, time_scale=2.0, preserve_envelope=False)
    off = float(np.abs(ind[:N] - want).max() / np.abs(want).max())
    print("closed form, independent at rho 2:", off)
    assert off > 0.1


def test_split_ranges_and_noise_are_bit_exact(amd, synth16k_fresh):
    from eaqhm_amd.model import noise_time_map, noise_time_map_contour, contour_time_map
    s_recon, _, arrays = synth16k_fresh
    L, n = len(s_recon), len(arrays["ti"])
    x = np.arange(n) / (n - 1)
    rng = np.random.default_rng(5)
    nz = amd.eaQHMNoiseAnalysis(s_recon + 1e-3 * rng.standard_normal(L), s_recon, 16000)
    for rho, beta in ((1.7, 0.9), (0.9 + 0.4 * x, 1.2 - 0.3 * x)):
        a = amd.eaQHMSynthesis(arrays, 16000, L, time_scale=rho, pitch_scale=beta, phase="shape")
        Lo = len(a)
        cuts = [(0, Lo // 3), (Lo // 3, Lo // 3 + 1001), (Lo // 3 + 1001, Lo)]
        split = amd.eaQHMSynthesis(arrays, 16000, L, time_scale=rho, pitch_scale=beta, phase="shape", _ranges=cuts)
        assert np.array_equal(split, a)
        both = amd.eaQHMSynthesis(arrays, 16000, L, time_scale=rho, pitch_scale=beta, phase="shape", noise=nz,
                                  noise_seed=11)
        if np.ndim(rho):
            tau = noise_time_map_contour(nz["hop"], contour_time_map(rho, beta, 15, L), 15)
        else:
            tau = noise_time_map(nz["hop"], Lo, rho)
        noise = amd.eaQHMNoiseSynthesis(nz, tau, Lo, seed=11)
        assert np.array_equal(both, a + noise)
        assert not np.array_equal(a, amd.eaQHMSynthesis(arrays, 16000, L, time_scale=rho, pitch_scale=beta))


def test_cli_phase_shape_writes_modified_wav(amd, tmp_path):
    import shutil
    from eaqhm_amd import cli
    wav = str(tmp_path / "SA19.WAV")
    shutil.copy(os.path.join(GOLDEN, "SA19.WAV"), wav)
    assert cli.main([wav, "--gender", "female", "--max-adpt", "1", "--phase", "shape", "--time-scale", "2"]) == 0
    fs, y = wavfile.read(str(tmp_path / "SA19_modified.wav"))
    _, _, det, _ = amd.eaQHMAnalysisAndSynthesis(wav, "female", maxAdpt=1, printPrompts=False)
    want = amd.eaQHMSynthesis(det, 16000, 63488, time_scale=2.0, phase="shape")
    assert fs == 16000 and y.dtype == np.float32 and y.shape == want.shape == (2 * 63488,)
    assert np.array_equal(y, np.float32(want))
    other = amd.eaQHMSynthesis(det, 16000, 63488, time_scale=2.0)
    assert not np.array_equal(np.float32(other), y)
