"""The formant scale on the MI355X (eaQHMSynthesis(formant_scale=...) -> eaqhm_modify_prep with alpha, and
model_envelope -> eaqhm_model_envelope): bit-identity with the four prep kernels the one prep kernel replaced and with
the synthesis as it was then (digests recorded on the MI355X at that commit, tests/golden/modify_parent_digests.json),
agreement with the NumPy model of DESIGN.md §9.2 (tests/model_formant_ref.py), the envelope readout, a hand-built
model whose formant moves where the definition says, the CLI and the probe's numbers."""
import hashlib
import json
import os

import numpy as np
import pytest
from scipy.io import wavfile

import model_formant_ref as MF
from conftest import GOLDEN, ROOT, record_measurement
from test_gpu_model_synthesis import analyse, reference_model

pytestmark = pytest.mark.gpu

SETTINGS = [(rho, beta, alpha) for alpha in (0.8, 1.25) for beta in (1.0, 1.25) for rho in (0.5, 1.0)]


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


@pytest.fixture(scope="module")
def synth16k_fresh(amd, tmp_path_factory):
    from eaqhm_amd.synth import synth_speech_int16
    return analyse(amd, tmp_path_factory.mktemp("f16"), synth_speech_int16(2.0, 16000), 16000, "synth16k_2s")


@pytest.fixture(scope="module")
def synth48k_fresh(amd, tmp_path_factory):
    from eaqhm_amd.synth import synth_speech_int16
    return analyse(amd, tmp_path_factory.mktemp("f48"), synth_speech_int16(0.6, 48000), 48000, "synth48k_0p6s",
                   maxAdpt=1)


@pytest.fixture(scope="module")
def models(synth16k_fresh, synth48k_fresh):
    """(label, arrays model, fs, length): the reference's SA19 model, fresh 2 s at 16 kHz, 0.6 s at 48 kHz."""
    g, det = reference_model()
    s16, _, a16 = synth16k_fresh
    s48, _, a48 = synth48k_fresh
    return [("sa19", det, 16000, len(g["s_recon"])), ("synth16k_2s", a16, 16000, len(s16)),
            ("synth48k_0p6s", a48, 48000, len(s48))]


def _prep_outputs(amd, det, fs, beta, alpha=None, gain=None, envelope=True):
    """amp, R, ph0 of one prep call: beta a number or one value per instant, gain (contours) and alpha optional."""
    import torch
    from eaqhm_amd.functions import _ctx
    from eaqhm_amd.model import unpack_model
    m = unpack_model(det)
    c = _ctx(0)
    dev = c.device
    rec_h = m["records"]
    n, K, D = rec_h.shape[0], m["Kmax"], m["step"]
    rec = torch.as_tensor(rec_h, device=dev)
    code = torch.empty(n * K, dtype=torch.uint8, device=dev)
    mom = torch.empty(n * (K + 1), dtype=torch.float64, device=dev)
    amp, R, ph0 = (torch.empty(n * K, dtype=torch.float64, device=dev) for _ in range(3))
    c.spline_solve(rec, n, K, D, code, mom)

    def dv(x):
        return None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)

    beta_n = beta if np.ndim(beta) else np.full(n, beta)
    c.modify_prep(rec, code, mom, n, K, D, fs, dv(beta_n), dv(gain), dv(alpha), envelope, amp, R, ph0)
    return [x.cpu().numpy().reshape(n, K) for x in (amp, R, ph0)]


def _parent_digests():
    with open(os.path.join(GOLDEN, "modify_parent_digests.json")) as f:
        return json.load(f)


def _digest(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return dict(shape=list(a.shape), sha256=hashlib.sha256(a.tobytes()).hexdigest())


def _sa19_contours(n):
    """The rho / beta contour of the recorded contour cases and the alpha ramp 0.9 -> 1.2."""
    x = np.arange(n) / (n - 1)
    return 1.1 + 0.5 * np.sin(2 * np.pi * 3 * x), 0.8 + 0.5 * x, 0.9 + 0.3 * x


def test_unit_alpha_prep_is_todays_prep_bit_for_bit(amd):
    """eaqhm_modify_prep against amp, R and ph0 of the four entry points it replaced (eaqhm_modify_prep, _prep_curve,
    _prep_formant, _prep_formant_curve), recorded on the MI355X at the commit the fixture names, on the committed SA19
    model.  Cases that had no alpha are called both without one and with alpha = 1 per instant: the envelope nodes
    ordered in LDS and read at (beta f) / 1 give the bits of the global-memory count and its own lookup."""
    from eaqhm_amd.model import contour_time_map
    g, det = reference_model()
    fs, L = 16000, len(g["s_recon"])
    n = len(det["ti"])
    want = _parent_digests()
    assert (want["fs"], want["length"], want["No_ti"]) == (fs, L, n)
    rho_c, beta_c, alpha_c = _sa19_contours(n)
    gain_c = contour_time_map(rho_c, beta_c, int(det["ti"][1] - det["ti"][0]), L)["gain"]
    cases = [("scalar_beta%g_env1" % b, dict(beta=b)) for b in (1.0, 0.8, 1.25, 1.9)]
    cases += [("scalar_beta%g_env0" % b, dict(beta=b, envelope=False)) for b in (1.0, 1.25)]
    cases += [("contour_env1", dict(beta=beta_c, gain=gain_c))]
    cases += [("formant_beta%g_alpha%g" % (b, a), dict(beta=b, alpha=np.full(n, a)))
              for a in (0.8, 1.25) for b in (1.0, 1.25)]
    cases += [("formant_contour", dict(beta=beta_c, gain=gain_c, alpha=alpha_c))]
    assert {k for k, _ in cases} == set(want["prep"])
    for key, kw in cases:
        forms = [("as recorded", kw)]
        if "alpha" not in kw and kw.get("envelope", True):      # alpha needs the envelope (EAQHM_EINVAL without)
            forms.append(("alpha = 1", dict(kw, alpha=np.ones(n))))
        for form, kw2 in forms:
            for x, name in zip(_prep_outputs(amd, det, fs, **kw2), ("amp", "R", "ph0")):
                assert _digest(x) == want["prep"][key][name], (key, form, name)


def test_synthesis_is_the_parents_bit_for_bit(amd):
    """eaQHMSynthesis and model_envelope on the committed SA19 model against the digests recorded on the MI355X before
    the four prep kernels became one: scalar (rho, beta, envelope), the three contour pairs of the test below, the
    formant SETTINGS, a formant contour, and the envelope readout on a 120-point grid."""
    g, det = reference_model()
    fs, L = 16000, len(g["s_recon"])
    n = len(det["ti"])
    want = _parent_digests()["synthesis"]
    x = np.arange(n) / (n - 1)
    rho_c, beta_c, alpha_c = _sa19_contours(n)
    cases = [("scalar_rho%g_beta%g_env%d" % (rho, b, env),
              dict(time_scale=rho, pitch_scale=b, preserve_envelope=env))
             for rho in (0.5, 1.0, 1.5) for b in (1.0, 0.8, 1.25) for env in (True, False)]
    cases += [("contour_rho_sinus", dict(time_scale=1.1 + 0.5 * np.sin(2 * np.pi * 3 * x), pitch_scale=np.ones(n))),
              ("contour_beta_ramp", dict(time_scale=np.ones(n), pitch_scale=0.8 + 0.5 * x)),
              ("contour_both", dict(time_scale=0.9 + 0.4 * x, pitch_scale=1.3 - 0.5 * x))]
    cases += [("formant_rho%g_beta%g_alpha%g" % (rho, b, a), dict(time_scale=rho, pitch_scale=b, formant_scale=a))
              for rho, b, a in SETTINGS]
    cases += [("formant_contour", dict(time_scale=rho_c, pitch_scale=beta_c, formant_scale=alpha_c))]
    got = {key: _digest(amd.eaQHMSynthesis(det, fs, L, **kw)) for key, kw in cases}
    grid = np.linspace(0.0, fs / 2, 120)
    for a in (1.0, 1.25):
        got["envelope_alpha%g" % a] = _digest(amd.model_envelope(det, fs, grid, formant_scale=a))
    assert set(got) == set(want)
    for key in sorted(want):
        assert got[key] == want[key], key


def test_unit_alpha_contour_is_todays_contour_path_bit_for_bit(amd, models):
    for label, det, fs, L in models:
        n = len(det["ti"])
        x = np.arange(n) / (n - 1)
        for rho, beta in ((1.1 + 0.5 * np.sin(2 * np.pi * 3 * x), np.ones(n)), (np.ones(n), 0.8 + 0.5 * x),
                          (0.9 + 0.4 * x, 1.3 - 0.5 * x)):
            ref = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta)
            out = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, formant_scale=np.ones(n))
            assert np.array_equal(out, ref), label
        # a number 1 is today's scalar path, call for call
        ref = amd.eaQHMSynthesis(det, fs, L, time_scale=1.5, pitch_scale=1.2)
        assert np.array_equal(amd.eaQHMSynthesis(det, fs, L, time_scale=1.5, pitch_scale=1.2, formant_scale=1.0), ref)


def test_gpu_against_numpy_formant_model(amd, models):
    """alpha in {0.8, 1.25} x beta in {1, 1.25} x rho in {0.5, 1}: the bar of test_gpu_model_synthesis (1e-8 of the
    maximum)."""
    from eaqhm_amd.model import unpack_model
    for label, det, fs, L in models:
        m = unpack_model(det)
        for rho, beta, alpha in SETTINGS:
            out = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, formant_scale=alpha)
            ref = MF.synthesize_formant(m["records"], m["step"], fs, L, rho, beta, alpha)
            assert out.shape == ref.shape == (int(np.rint(rho * L)),)
            rel = float(np.abs(out - ref).max() / np.abs(ref).max())
            record_measurement("model_formant_vs_numpy_%s_rho%g_beta%g_alpha%g" % (label, rho, beta, alpha),
                               max_rel=rel)
            assert rel <= 1e-8, (label, rho, beta, alpha, rel)


def test_gpu_against_numpy_formant_contour(amd, models):
    """alpha ramping 0.9 -> 1.2 over the model, alone and with rho and beta contours (the contour bar, 1e-8)."""
    from eaqhm_amd.model import unpack_model
    for label, det, fs, L in models:
        m = unpack_model(det)
        n = len(m["records"])
        x = np.arange(n) / (n - 1)
        alpha = 0.9 + 0.3 * x
        for name, rho, beta in (("alpha_ramp", 1.0, 1.0), ("all", 1.1 + 0.4 * np.sin(2 * np.pi * 2 * x), 1.25 - 0.3 * x)):
            out = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, formant_scale=alpha)
            ref = MF.synthesize_formant_contour(m["records"], m["step"], fs, L, rho, beta, alpha)
            assert out.shape == ref.shape
            rel = float(np.abs(out - ref).max() / np.abs(ref).max())
            record_measurement("model_formant_contour_vs_numpy_%s_%s" % (label, name), max_rel=rel)
            assert rel <= 1e-8, (label, name, rel)


def test_model_envelope_against_numpy(amd, models):
    """1e-12 absolute in log amplitude; the grid holds node frequencies exactly (ties) and points beyond the nodes."""
    from eaqhm_amd.model import unpack_model
    for label, det, fs, L in models:
        m = unpack_model(det)
        rec, K = m["records"], m["Kmax"]
        n = len(rec)
        fm = rec[:, K:2 * K]
        nodes = np.unique(fm[fm > 0])
        pick = nodes[np.linspace(0, len(nodes) - 1, 200).astype(int)]
        grid = np.unique(np.concatenate((np.linspace(0.0, fs / 2, 301), pick, [0.0, fs])))
        for alpha in (1.0, 1.3, 0.75, 0.6 + 0.8 * np.arange(n) / (n - 1)):
            out = amd.model_envelope(det, fs, grid, formant_scale=alpha)
            ref = MF.envelope_readout(rec, grid, alpha)
            assert out.shape == ref.shape == (n, len(grid))
            inf = np.isneginf(ref)
            assert np.array_equal(np.isneginf(out), inf)
            err = float(np.abs(out[~inf] - ref[~inf]).max())
            record_measurement("model_envelope_vs_numpy_%s_alpha%s" % (label, "contour" if np.ndim(alpha) else alpha),
                               max_abs=err)
            assert err <= 1e-12, (label, err)


def _harmonic_model(n=201, D=80, fs=16000, f0=100.0, H=60):
    """f0 = 100 Hz held, 60 harmonics with consistent phases, log amplitudes with a Gaussian bump at 1000 Hz."""
    ti = np.arange(n) * D
    k = np.arange(1, H + 1)
    f = f0 * k
    lna = np.log(0.01) + 3.0 * np.exp(-0.5 * ((f - 1000.0) / 250.0) ** 2)
    ph = np.angle(np.exp(1j * 2 * np.pi * f[None, :] * ti[:, None] / fs))
    det = dict(ti=ti, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=np.tile(np.exp(lna), (n, 1)),
               frange=np.tile(f, (n, 1)), pk=ph)
    return det, (n - 1) * D + 1, f


def test_formant_moves_where_the_definition_says(amd):
    from eaqhm_amd.model import unpack_model
    fs, f0 = 16000, 100.0
    det, L, f = _harmonic_model(fs=fs, f0=f0)
    base = amd.eaQHMSynthesis(det, fs, L)
    assert np.array_equal(amd.eaQHMSynthesis(det, fs, L, formant_scale=1.0), base)
    n = len(det["ti"])
    assert np.array_equal(amd.eaQHMSynthesis(det, fs, L, time_scale=np.ones(n), formant_scale=np.ones(n)),
                          amd.eaQHMSynthesis(det, fs, L, time_scale=np.ones(n)))
    out = amd.eaQHMSynthesis(det, fs, L, formant_scale=1.3)
    assert out.shape == base.shape
    t = np.arange(4000, 12000)                                  # steady: away from the ends of the runs
    cols = [np.cos(2 * np.pi * fk * t / fs) for fk in f] + [np.sin(2 * np.pi * fk * t / fs) for fk in f]
    X = np.stack(cols, axis=1)
    coef, *_ = np.linalg.lstsq(X, out[t], rcond=None)
    amps = np.hypot(coef[:len(f)], coef[len(f):])
    assert int(np.argmax(amps)) + 1 == 13
    rec = unpack_model(det)["records"]
    want = 2.0 * np.exp(MF.envelope_readout(rec[:1], f / 1.3, 1.0)[0])
    rel = float(np.abs(amps / want - 1.0).max())
    record_measurement("model_formant_harmonic_fit", max_rel=rel)
    assert rel <= 1e-6


def test_cli_formant_scale_writes_modified_wav(amd, tmp_path):
    import shutil
    from eaqhm_amd import cli
    wav = str(tmp_path / "SA19.WAV")
    shutil.copy(os.path.join(GOLDEN, "SA19.WAV"), wav)
    assert cli.main([wav, "--gender", "female", "--max-adpt", "1", "--formant-scale", "1.2"]) == 0
    fs, y = wavfile.read(str(tmp_path / "SA19_modified.wav"))
    _, x = wavfile.read(wav)
    assert fs == 16000 and y.dtype == np.float32 and y.shape == x.shape
    assert np.all(np.isfinite(y)) and np.abs(y).max() > 0.01


def test_record_probe_numbers(amd, synth16k_fresh, synth48k_fresh):
    """Device times of the formant prep + scan against today's scalar prep on the fresh models (evidence, not
    assertions; the 60 s numbers come from tools/model_synthesis_probe.py --formant)."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from model_synthesis_probe import formant_rows, prepare
    for label, (s, _, arrays), fs in (("synth16k_2s", synth16k_fresh, 16000), ("synth48k_0p6s", synth48k_fresh, 48000)):
        st = prepare(torch, arrays, fs, len(s), reps=5)
        for row in formant_rows(torch, st, reps=5):
            record_measurement("model_formant_probe_%s_%s" % (label, row["setting"]),
                               **{k: v for k, v in row.items() if k != "setting"})
            assert row["prep_scan_ms"] > 0 and row["eval_ms"] > 0
