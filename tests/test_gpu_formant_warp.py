"""The piecewise-linear formant warp on the MI355X (eaQHMSynthesis(formant_warp=...) -> eaqhm_modify_amp_warp,
model_envelope -> eaqhm_model_envelope_warp, eaQHMNoiseWarp -> eaqhm_noise_warp_map, noise_envelope ->
eaqhm_noise_envelope_map) against the NumPy model of DESIGN.md §9.4 and §10.3 (tests/formant_warp_ref.py).

Bars.  Synthesis: 1e-8 of the peak, the bar of test_gpu_model_synthesis and test_gpu_model_formant.  Envelope readout:
1e-12 absolute in log amplitude, the existing readout bar.  Noise warp and noise envelope: §10's rule, at most 100 x
the largest deviation between the model run in float64 and in np.longdouble on the same input, computed when the test
runs; only frames whose stop stage differs between those two runs may be left out (at most 1 % of the non-silent
frames, none on AR(4))."""
import os

import numpy as np
import pytest
from scipy.io import wavfile

import formant_warp_ref as FW
import noise_model_ref as N
from conftest import GOLDEN, load_golden, record_measurement
from test_gpu_model_formant import _harmonic_model
from test_gpu_model_synthesis import analyse, reference_model

pytestmark = pytest.mark.gpu

SETTINGS = [(rho, beta) for beta in (1.0, 1.25) for rho in (0.5, 1.0)]


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


def _on(x_new, x, y):
    """The map (x, y) given on the breakpoints x_new instead (x_new holds x's breakpoints)."""
    return np.asarray(FW.warp_forward(x, y, x_new), dtype=np.float64)


def maps(fs, n):
    """(label, f_in [B], f_out [B] or [n, B]) in Hz: VTLN 0.8 and 1.25, three breakpoints, B = 16, B = 1, and a ramp
    over the n rows between the two VTLN maps (on the union of their breakpoints)."""
    nyq = fs / 2.0
    x16 = nyq * np.arange(1, 17) / 16.0
    y16 = x16 * (1.0 + 0.15 * np.sin(np.pi * np.arange(1, 17) / 16.0))
    lo, hi = FW.vtln(fs, 0.8), FW.vtln(fs, 1.25)
    xu = np.array([hi[0][0], lo[0][0], nyq])
    u = (np.arange(n) / (n - 1.0))[:, None]
    ramp = (1 - u) * _on(xu, *lo) + u * _on(xu, *hi)
    ramp[:, 2] = nyq
    return [("vtln0.8",) + lo, ("vtln1.25",) + hi,
            ("three", np.array([0.125, 0.375, 0.75]) * nyq, np.array([0.15, 0.4375, 0.8]) * nyq),
            ("b16", x16, y16), ("b1", np.array([1000.0]), np.array([1180.0])), ("ramp", xu, ramp)]


# ---- the deterministic part
@pytest.fixture(scope="module")
def models(amd, tmp_path_factory):
    """label -> (arrays model, fs, length): the reference's SA19 model, fresh 2 s at 16 kHz, 0.6 s at 48 kHz (Kmax 148:
    three lane chunks)."""
    from eaqhm_amd.synth import synth_speech_int16
    g, det = reference_model()
    x16, x48 = synth_speech_int16(2.0, 16000), synth_speech_int16(0.6, 48000)
    _, _, a16 = analyse(amd, tmp_path_factory.mktemp("fw16"), x16, 16000, "synth16k_2s")
    _, _, a48 = analyse(amd, tmp_path_factory.mktemp("fw48"), x48, 48000, "synth48k_0p6s", maxAdpt=1)
    assert np.asarray(a48["amplitudes"]).shape[1] > 64
    return {"sa19": (det, 16000, len(g["s_recon"])), "synth16k_2s": (a16, 16000, len(x16)),
            "synth48k_0p6s": (a48, 48000, len(x48))}


HAND_X = np.array([1000.0, 3000.0, 6000.0])
HAND_Y = np.array([1200.0, 3500.0, 6400.0])


def hand_model():
    """9 instants (not a multiple of the 4 waves of a block), Kmax 5, step 80 at 16 kHz.  Slots at 400, 2800, 3000,
    3000 (tied nodes) and 7000 Hz; instant 4 has no active partial; slot 0 is missing at instant 6.  With the map
    (HAND_X, HAND_Y) and beta = 1.25 the partial at 2800 Hz reads at 3500 Hz = y_1 exactly, where V = x_1 = 3000 Hz is
    exactly the tied nodes' frequency; the partial at 7000 Hz reads beyond y_2 at beta = 1 and lies past Nyquist at
    beta = 1.25."""
    n, D, fs = 9, 80, 16000
    ti = np.arange(n) * D
    f = np.array([400.0, 2800.0, 3000.0, 3000.0, 7000.0])
    lna = np.array([-3.0, -4.5, -3.5, -5.0, -6.0])[None, :] + 0.05 * np.arange(n)[:, None]
    am = np.exp(lna)
    fm = np.tile(f, (n, 1))
    ph = np.angle(np.exp(1j * 2 * np.pi * f[None, :] * ti[:, None] / fs)) + 0.3 * np.arange(5)[None, :]
    am[4] = 0.0
    am[6, 0] = 0.0
    det = dict(ti=ti, isVoiced=np.ones(n, bool), a0=0.001 * np.arange(n), amplitudes=am, frange=fm, pk=ph)
    return det, fs, (n - 1) * D + 1


def _check_synthesis(amd, label, det, fs, L, name, x, y, rho, beta):
    from eaqhm_amd.model import unpack_model
    m = unpack_model(det)
    out = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, formant_warp=(x, y))
    ref = FW.synthesize(m["records"], m["step"], fs, L, rho, beta, x, y)
    assert out.shape == ref.shape == (int(np.rint(rho * L)),) and out.dtype == np.float64
    rel = float(np.abs(out - ref).max() / np.abs(ref).max())
    print("formant warp %s %s rho %g beta %g: max rel %.3g" % (label, name, rho, beta, rel))
    record_measurement("formant_warp_vs_numpy_%s_%s_rho%g_beta%g" % (label, name, rho, beta), max_rel=rel)
    assert rel <= 1e-8, (label, name, rho, beta, rel)
    return out


@pytest.mark.parametrize("label", ["sa19", "synth16k_2s", "synth48k_0p6s"])
def test_synthesis_against_numpy_model(amd, models, label):
    """Every map on every model, the four (rho, beta) settings dealt over the maps (a different deal per model, so the
    three models together put every map at three settings); the hand-built model below takes the full product."""
    det, fs, L = models[label]
    n = len(det["ti"])
    shift = ["sa19", "synth16k_2s", "synth48k_0p6s"].index(label)
    for j, (name, x, y) in enumerate(maps(fs, n)):
        rho, beta = SETTINGS[(j + shift) % 4]
        _check_synthesis(amd, label, det, fs, L, name, x, y, rho, beta)


def test_synthesis_hand_built_model(amd):
    det, fs, L = hand_model()
    n = len(det["ti"])
    for name, x, y in maps(fs, n) + [("hand", HAND_X, HAND_Y)]:
        for rho, beta in SETTINGS:
            _check_synthesis(amd, "hand", det, fs, L, name, x, y, rho, beta)
    # a contour of rho selects the contour path; the per-instant rows ride along
    name, x, y = maps(fs, n)[5]
    rho = np.linspace(0.8, 1.4, n)
    out = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=1.25, formant_warp=(x, y))
    from eaqhm_amd.model import unpack_model
    m = unpack_model(det)
    ref = FW.synthesize(m["records"], m["step"], fs, L, rho, 1.25, x, y)
    assert out.shape == ref.shape
    rel = float(np.abs(out - ref).max() / np.abs(ref).max())
    record_measurement("formant_warp_vs_numpy_hand_contour", max_rel=rel)
    assert rel <= 1e-8, rel


def test_hand_built_amplitudes_hit_the_edge_cases(amd):
    """The amplitudes the kernel wrote, read back through a call of the entry point itself, against the model: the
    inactive instant, the tied nodes, the read on a node and on a breakpoint, the read beyond the last breakpoint and
    the partial past Nyquist."""
    import torch
    from eaqhm_amd.functions import _ctx
    from eaqhm_amd.model import unpack_model
    det, fs, L = hand_model()
    m = unpack_model(det)
    rec_h, K, n = m["records"], m["Kmax"], len(m["records"])
    c = _ctx(0)
    rec = torch.as_tensor(rec_h, device=c.device)
    x_d, y_d = (torch.as_tensor(v, device=c.device) for v in (HAND_X, np.tile(HAND_Y, (n, 1))))
    for beta in (1.0, 1.25):
        amp = torch.full((n, K), -1.0, dtype=torch.float64, device=c.device)
        c.modify_amp_warp(rec, n, K, float(fs), torch.full((n,), beta, dtype=torch.float64, device=c.device), x_d, y_d,
                          3, amp)
        got = amp.cpu().numpy()
        ref = FW.amplitudes(rec_h[:, :K], rec_h[:, K:2 * K], fs, beta, HAND_X, HAND_Y)
        assert np.array_equal(got == 0, ref == 0) and np.all(got[4] == 0) and got[6, 0] == 0
        live = ref != 0
        err = float(np.abs(np.log(got[live]) - np.log(ref[live])).max())
        record_measurement("formant_warp_hand_amplitudes_beta%g" % beta, max_abs_log=err)
        assert err <= 1e-12
        if beta == 1.25:
            assert FW.warp_inverse(HAND_X, HAND_Y, 1.25 * 2800.0) == 3000.0      # on y_1 -> x_1: the tied nodes
            assert np.all(got[:, 4] == 0)                                         # 8750 Hz: past Nyquist
            keep = np.r_[0:4, 5:9]
            assert np.abs(np.log(got[keep, 1]) - np.log(rec_h[keep, 2])).max() <= 1e-12   # the first of the tied nodes
    # an identity row and beta == 1: a copy
    amp = torch.full((n, K), -1.0, dtype=torch.float64, device=c.device)
    c.modify_amp_warp(rec, n, K, float(fs), torch.ones(n, dtype=torch.float64, device=c.device), x_d,
                      torch.as_tensor(np.tile(HAND_X, (n, 1)), device=c.device), 3, amp)
    assert np.array_equal(amp.cpu().numpy(), rec_h[:, :K])


def test_model_envelope_against_numpy(amd, models):
    """1e-12 absolute in log amplitude; the grid holds node frequencies, breakpoints y_j exactly, and points beyond the
    nodes and beyond the last breakpoint; rows of empty instants are -inf."""
    from eaqhm_amd.model import unpack_model
    cases = [(k,) + v for k, v in models.items()] + [("hand",) + hand_model()]
    for label, det, fs, L in cases:
        m = unpack_model(det)
        rec, K = m["records"], m["Kmax"]
        n = len(rec)
        fm = rec[:, K:2 * K]
        nodes = np.unique(fm[fm > 0])
        pick = nodes[np.linspace(0, len(nodes) - 1, 60).astype(int)]
        every = maps(fs, n) + ([("hand", HAND_X, HAND_Y)] if label == "hand" else [])
        for name, x, y in every:
            grid = np.unique(np.concatenate((np.linspace(0.0, fs / 2, 131), pick, np.ravel(y)[:32], [0.0, 0.7 * fs])))
            out = amd.model_envelope(det, fs, grid, formant_warp=(x, y))
            ref = FW.envelope_readout(rec, grid, x, y)
            assert out.shape == ref.shape == (n, len(grid)) and out.dtype == np.float64
            inf = np.isneginf(ref)
            assert np.array_equal(np.isneginf(out), inf)
            if label == "hand":
                assert inf[4].all() and not inf[[0, 8]].any()
            err = float(np.abs(out[~inf] - ref[~inf]).max())
            record_measurement("formant_warp_envelope_vs_numpy_%s_%s" % (label, name), max_abs=err)
            assert err <= 1e-12, (label, name, err)
        # the identity map is the plain readout, bit for bit
        grid = np.linspace(0.0, fs / 2, 50)
        x = maps(fs, n)[2][1]
        assert np.array_equal(amd.model_envelope(det, fs, grid, formant_warp=(x, x.copy())),
                              amd.model_envelope(det, fs, grid)), label


def test_identity_map(amd, models):
    """beta = 1: bit for bit the call without a warp; beta != 1: within the synthesis bar of it (the same envelope read
    at the same frequency)."""
    det, fs, L = models["sa19"]
    hand = hand_model()
    for label, (d, f, l) in (("sa19", (det, fs, L)), ("hand", hand)):
        n = len(d["ti"])
        x = maps(f, n)[2][1]
        for y in (x.copy(), np.tile(x, (n, 1))):
            for rho in (0.5, 1.0):
                assert np.array_equal(amd.eaQHMSynthesis(d, f, l, time_scale=rho, formant_warp=(x, y)),
                                      amd.eaQHMSynthesis(d, f, l, time_scale=rho)), (label, rho)
            out = amd.eaQHMSynthesis(d, f, l, pitch_scale=1.25, formant_warp=(x, y))
            ref = amd.eaQHMSynthesis(d, f, l, pitch_scale=1.25)
            rel = float(np.abs(out - ref).max() / np.abs(ref).max())
            record_measurement("formant_warp_identity_beta1.25_%s_%s" % (label, "rows" if y.ndim == 2 else "row"),
                               max_rel=rel)
            assert rel <= 1e-8, (label, rel)
    assert np.array_equal(amd.eaQHMSynthesis(det, fs, L, formant_warp=None), amd.eaQHMSynthesis(det, fs, L))


def test_one_breakpoint_is_the_formant_scale(amd, models):
    for label, (det, fs, L) in models.items():
        for alpha, rho, beta in ((0.8, 1.0, 1.25), (1.25, 0.5, 1.0)):
            x = np.array([1000.0])
            out = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, formant_warp=(x, alpha * x))
            ref = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, formant_scale=alpha)
            rel = float(np.abs(out - ref).max() / np.abs(ref).max())
            record_measurement("formant_warp_b1_vs_scale_%s_alpha%g" % (label, alpha), max_rel=rel)
            assert out.shape == ref.shape and rel <= 1e-8, (label, alpha, rel)


def test_formant_peak_moves_to_W_of_F(amd):
    """The harmonic model of test_gpu_model_formant (f0 = 100 Hz, a bump at 1000 Hz) under a three-breakpoint map with
    W(1000) = 1200: the fitted harmonic amplitudes are exp(E(V(f))) and peak at harmonic 12.  Under a VTLN map the
    envelope at fs/2 is the model's at fs/2, which the scale alpha = 1.25 does not give."""
    from eaqhm_amd.model import unpack_model
    fs = 16000
    det, L, f = _harmonic_model(fs=fs, f0=100.0)
    x, y = np.array([1000.0, 3000.0, 8000.0]), np.array([1200.0, 3300.0, 8000.0])
    assert FW.warp_forward(x, y, np.array([1000.0]))[0] == 1200.0
    out = amd.eaQHMSynthesis(det, fs, L, formant_warp=(x, y))
    t = np.arange(4000, 12000)
    X = np.stack([np.cos(2 * np.pi * fk * t / fs) for fk in f] + [np.sin(2 * np.pi * fk * t / fs) for fk in f], axis=1)
    coef, *_ = np.linalg.lstsq(X, out[t], rcond=None)
    amps = np.hypot(coef[:len(f)], coef[len(f):])
    assert int(np.argmax(amps)) + 1 == 12
    rec = unpack_model(det)["records"]
    want = 2.0 * np.exp(FW.envelope_readout(rec[:1], f, x, y)[0])
    rel = float(np.abs(amps / want - 1.0).max())
    record_measurement("formant_warp_harmonic_fit", max_rel=rel)
    assert rel <= 1e-6
    for d, fs_ in ((det, fs), hand_model()[:2]):
        top = np.array([fs_ / 2.0])
        base = amd.model_envelope(d, fs_, top)
        for alpha in (0.8, 1.25):
            assert np.array_equal(amd.model_envelope(d, fs_, top, formant_warp=FW.vtln(fs_, alpha)), base)
    d, fs_ = hand_model()[:2]      # its top node lies at 7000 Hz: the scale 1.25 reads fs/2 at 6400 Hz, inside the band
    base = amd.model_envelope(d, fs_, [fs_ / 2.0])
    scaled = amd.model_envelope(d, fs_, [fs_ / 2.0], formant_scale=1.25)
    fin = np.isfinite(base)
    assert fin.sum() == 8 and np.all(scaled[fin] != base[fin])


# ---- the noise
def _trim(nz, lo, hi):
    """Frames [lo, hi) of a noise model as a model of its own (frames are warped independently of each other)."""
    return dict(nz, sigma=nz["sigma"][lo:hi].copy(), refl=nz["refl"][lo:hi].copy(),
                length=(hi - lo - 1) * nz["hop"] + 1)


@pytest.fixture(scope="module")
def sa19(amd, tmp_path_factory):
    g = load_golden("sa19_female_default.npz")
    path = os.path.join(GOLDEN, "SA19.WAV")
    fs, x = wavfile.read(path)
    s_recon, _, arrays = analyse(amd, tmp_path_factory.mktemp("fw19"), x, fs, "SA19", track=g["swipe_track"])
    fs2, s = amd.read_signal(path)
    assert fs2 == fs == 16000 and len(s) == len(s_recon)
    return s, s_recon, arrays


@pytest.fixture(scope="module")
def noise_models(amd, sa19, tmp_path_factory):
    """label -> noise model: AR(4) (frames 120..277: the silent stretch and both sides of it), the SA19 residual (301
    frames from the middle), 0.6 s at 48 kHz with p = 50.  No frame count is a multiple of the 8 waves of a block."""
    from eaqhm_amd.synth import synth_speech_int16
    e = N.ar_fixture()
    x = synth_speech_int16(0.6, 48000)
    r48, _, _ = analyse(amd, tmp_path_factory.mktemp("fwn48"), x, 48000, "synth48k_0p6s", maxAdpt=1)
    ar = amd.eaQHMNoiseAnalysis(e, np.zeros(len(e)), 16000)
    s19 = amd.eaQHMNoiseAnalysis(sa19[0], sa19[1], 16000)
    n48 = amd.eaQHMNoiseAnalysis(x / 32768.0, r48, 48000)
    mid = len(s19["sigma"]) // 2
    out = {"ar4": _trim(ar, 120, 277), "sa19": _trim(s19, mid - 150, mid + 151),
           "synth48k": n48 if len(n48["sigma"]) % 8 else _trim(n48, 0, len(n48["sigma"]) - 3)}
    assert [(nz["hop"], nz["order"]) for nz in out.values()] == [(80, 18), (80, 18), (240, 50)]
    assert all(len(nz["sigma"]) % 8 for nz in out.values()) and np.any(out["ar4"]["sigma"] == 0)
    return out


MAP_NAMES = ["vtln0.8", "vtln1.25", "three", "b16", "b1", "ramp"]


@pytest.mark.parametrize("name", MAP_NAMES)
@pytest.mark.parametrize("label", ["ar4", "sa19", "synth48k"])
def test_noise_warp_against_numpy_model(amd, noise_models, label, name):
    nz = noise_models[label]
    Nf, fs = len(nz["sigma"]), nz["fs"]
    _, x, y = maps(fs, Nf)[MAP_NAMES.index(name)]
    live = nz["sigma"] > 0
    smax = float(nz["sigma"].max())
    got = amd.eaQHMNoiseWarp(nz, formant_warp=(x, y))
    assert {k: got[k] for k in ("hop", "order", "fs", "length")} == {k: nz[k] for k in ("hop", "order", "fs", "length")}
    assert got["sigma"].shape == (Nf,) and got["refl"].shape == nz["refl"].shape
    assert got["sigma"].dtype == got["refl"].dtype == np.float64
    sg, k, stop = FW.noise_warp(nz["sigma"], nz["refl"], x / fs, y / fs)
    sg_l, k_l, stop_l = FW.noise_warp(nz["sigma"], nz["refl"], x / fs, y / fs, np.longdouble)
    assert np.array_equal(got["sigma"] == 0, ~live) and np.all(got["refl"][~live] == 0)      # silent stays silent
    keep = stop == stop_l
    excluded = int(np.count_nonzero(~keep))
    dev_k = float(np.abs(k[keep] - k_l[keep]).max())
    dev_s = float(np.abs(sg[keep] - sg_l[keep]).max() / smax)
    err_k = float(np.abs(got["refl"][keep] - k[keep]).max())
    err_s = float(np.abs(got["sigma"][keep] - sg[keep]).max() / smax)
    print("noise warp map %s %s: frames %d silent %d stopped early %d excluded %d  k: model dev %.3g gpu err %.3g  "
          "sigma: model dev %.3g gpu err %.3g" % (label, name, Nf, int((~live).sum()), int((stop > 0).sum()), excluded,
                                                  dev_k, err_k, dev_s, err_s))
    record_measurement("noise_warp_map_vs_numpy_%s_%s" % (label, name), frames=Nf, silent=int((~live).sum()),
                       stopped_early=int((stop > 0).sum()), excluded=excluded, model_dev_k=dev_k, gpu_err_k=err_k,
                       model_dev_sigma=dev_s, gpu_err_sigma=err_s)
    if label == "ar4":
        assert excluded == 0 and not stop.any()
    assert excluded <= 0.01 * int(live.sum()), (label, name, excluded)
    assert dev_k > 0 and dev_s > 0
    assert err_k <= 100 * dev_k, (label, name, err_k, dev_k)
    assert err_s <= 100 * dev_s, (label, name, err_s, dev_s)
    if name == "b1":      # B = 1 against formant_scale = alpha, under the same bar
        alt = amd.eaQHMNoiseWarp(nz, float(y[0] / x[0]))
        d_k = float(np.abs(got["refl"][keep] - alt["refl"][keep]).max())
        d_s = float(np.abs(got["sigma"][keep] - alt["sigma"][keep]).max() / smax)
        record_measurement("noise_warp_map_b1_vs_scale_%s" % label, diff_k=d_k, diff_sigma=d_s, model_dev_k=dev_k,
                           model_dev_sigma=dev_s)
        assert d_k <= 100 * dev_k and d_s <= 100 * dev_s, (label, d_k, d_s)


@pytest.mark.parametrize("label", ["ar4", "sa19", "synth48k"])
def test_noise_envelope_against_numpy_model(amd, noise_models, label):
    nz = noise_models[label]
    Nf, fs = len(nz["sigma"]), nz["fs"]
    for name, x, y in maps(fs, Nf):
        freqs = np.concatenate((np.linspace(0.0, fs / 2, 65), np.ravel(y)[:16], [0.6 * fs, 3 * fs]))
        got = amd.noise_envelope(nz, fs, freqs, formant_warp=(x, y))
        ref = FW.noise_envelope(nz["sigma"], nz["refl"], x / fs, y / fs, freqs / fs)
        ref_l = FW.noise_envelope(nz["sigma"], nz["refl"], x / fs, y / fs, freqs / fs, np.longdouble)
        assert got.shape == ref.shape == (Nf, len(freqs)) and got.dtype == np.float64
        fin = np.isfinite(ref)
        assert np.array_equal(np.isneginf(got), ~fin) and np.array_equal(fin.all(axis=1), nz["sigma"] > 0)
        dev = float(np.abs(ref[fin] - ref_l[fin]).max())
        err = float(np.abs(got[fin] - ref[fin]).max())
        print("noise envelope map %s %s: model dev %.3g gpu err %.3g" % (label, name, dev, err))
        record_measurement("noise_envelope_map_vs_numpy_%s_%s" % (label, name), model_dev=dev, gpu_err=err)
        assert dev > 0 and err <= 100 * dev, (label, name, err, dev)


def test_noise_identity_rows_return_the_input(amd, noise_models):
    for label, nz in noise_models.items():
        Nf, fs = len(nz["sigma"]), nz["fs"]
        _, x, y = maps(fs, Nf)[5]
        got = amd.eaQHMNoiseWarp(nz, formant_warp=(x, x.copy()))
        assert np.array_equal(got["sigma"], nz["sigma"]) and np.array_equal(got["refl"], nz["refl"]), label
        assert got["sigma"] is not nz["sigma"]
        rows = y.copy()
        lo, hi = Nf // 4, Nf // 2
        rows[lo:hi] = x
        got = amd.eaQHMNoiseWarp(nz, formant_warp=(x, rows))
        assert np.array_equal(got["sigma"][lo:hi], nz["sigma"][lo:hi]), label
        assert np.array_equal(got["refl"][lo:hi], nz["refl"][lo:hi]), label
        rest = np.r_[0:lo, hi:Nf]
        rest = rest[nz["sigma"][rest] > 0]
        assert np.all(got["sigma"][rest] != nz["sigma"][rest]), label
        whole = amd.eaQHMNoiseWarp(nz, formant_warp=(x, y))
        assert np.array_equal(got["refl"][rest], whole["refl"][rest])       # a frame does not depend on its neighbours


def test_synthesis_with_noise_formant_is_the_prewarped_model(amd, sa19):
    s, s_recon, det = sa19
    fs, L = 16000, len(s)
    nz = amd.eaQHMNoiseAnalysis(s, s_recon, fs)
    n = len(det["ti"])
    every = maps(fs, n)
    rho_c = 1.1 + 0.5 * np.sin(2 * np.pi * 3 * np.arange(n) / (n - 1))
    for (name, x, y), kw in ((every[0], dict()), (every[5], dict(pitch_scale=1.7, time_scale=1.5)),
                             (every[2], dict(time_scale=rho_c)), (every[5], dict(phase="shape", time_scale=2.0))):
        warped = amd.eaQHMNoiseWarp(nz, formant_warp=amd.noise_formant_warp(nz, det, (x, y)))
        assert not np.array_equal(warped["refl"], nz["refl"])
        one = amd.eaQHMSynthesis(det, fs, L, noise=nz, noise_seed=9, noise_formant=True, formant_warp=(x, y), **kw)
        two = amd.eaQHMSynthesis(det, fs, L, noise=warped, noise_seed=9, formant_warp=(x, y), **kw)
        plain = amd.eaQHMSynthesis(det, fs, L, noise=nz, noise_seed=9, formant_warp=(x, y), **kw)
        assert np.array_equal(one, two), (name, sorted(kw))
        assert not np.array_equal(one, plain), (name, sorted(kw))
    c1, c2 = len(one) // 3, 2 * len(one) // 3 + 7
    parts = amd.eaQHMSynthesis(det, fs, L, noise=nz, noise_seed=9, noise_formant=True, formant_warp=(x, y),
                               _ranges=[(0, c1), (c1, c2), (c2, len(one))], **kw)
    assert np.array_equal(parts, one)


def test_entry_points_reject_bad_arguments(amd):
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)

    def z(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=c.device)

    Nf, p, F, B = 37, 4, 9, 2
    x = torch.as_tensor(np.array([0.2, 0.5]), device=c.device)      # B is refused before anything is read
    y = torch.as_tensor(np.tile([0.25, 0.5], (Nf, 1)), device=c.device)
    sigma, refl, so, ro, fn, out = z(Nf) + 0.1, z(Nf, 64), z(Nf), z(Nf, 64), z(F), z(Nf, F)
    n, K = 9, 5
    rec, beta, amp, env = z(n, 3 * K + 1), z(n) + 1.25, z(n, K), z(n, F)
    yi = torch.as_tensor(np.tile([0.25, 0.5], (n, 1)), device=c.device)
    good = {"noise_warp_map": [sigma, refl, Nf, p, x, y, B, so, ro],
            "noise_envelope_map": [sigma, refl, Nf, p, x, y, B, fn, F, out],
            "modify_amp_warp": [rec, n, K, 16000.0, beta, x, yi, B, amp],
            "model_envelope_warp": [rec, n, K, x, yi, B, fn, F, env]}
    for name, args in good.items():                                   # the good calls
        getattr(c, name)(*args)
    c.sync()
    assert torch.all(so > 0) and torch.all(out == out[0, 0])           # a white frame stays white
    assert torch.all(amp == 0) and torch.all(torch.isinf(env))         # an empty model: no amplitude, -inf rows
    b_at = {"noise_warp_map": 6, "noise_envelope_map": 6, "modify_amp_warp": 7, "model_envelope_warp": 5}
    for name, args in good.items():
        fn_ = getattr(c, name)
        for bad_b in (0, 17, -1):
            with pytest.raises(RuntimeError, match="error -1"):
                fn_(*[bad_b if j == b_at[name] else a for j, a in enumerate(args)])
        for j, a in enumerate(args):
            if torch.is_tensor(a):
                with pytest.raises(RuntimeError, match="error -1"):
                    fn_(*[None if i == j else v for i, v in enumerate(args)])
    for order in (0, 64):
        with pytest.raises(RuntimeError, match="error -1"):
            c.noise_warp_map(sigma, refl, Nf, order, x, y, B, so, ro)
        with pytest.raises(RuntimeError, match="error -1"):
            c.noise_envelope_map(sigma, refl, Nf, order, x, y, B, fn, F, out)
    with pytest.raises(RuntimeError, match="error -1"):
        c.noise_warp_map(sigma, refl, 0, p, x, y, B, so, ro)
    with pytest.raises(RuntimeError, match="error -1"):
        c.noise_envelope_map(sigma, refl, Nf, p, x, y, B, fn, 0, out)
    with pytest.raises(RuntimeError, match="error -1"):
        c.modify_amp_warp(rec, 3, K, 16000.0, beta, x, yi, B, amp)
    with pytest.raises(RuntimeError, match="error -1"):
        c.modify_amp_warp(rec, n, K, 0.0, beta, x, yi, B, amp)
    with pytest.raises(RuntimeError, match="error -1"):
        c.model_envelope_warp(rec, n, K, x, yi, B, fn, 0, env)
    with pytest.raises(RuntimeError, match="error -1"):
        c.model_envelope_warp(rec, n, 100000, x, yi, B, fn, F, env)
    assert c.abi_version == 6


def test_cli_formant_vtln_writes_modified(amd, tmp_path):
    import shutil
    from eaqhm_amd import cli
    wav = str(tmp_path / "SA19.WAV")
    shutil.copy(os.path.join(GOLDEN, "SA19.WAV"), wav)
    base = [wav, "--gender", "female", "--max-adpt", "1", "--noise", "--noise-seed", "3"]
    assert cli.main(base + ["--formant-vtln", "1.15"]) == 0
    _, plain = wavfile.read(str(tmp_path / "SA19_modified.wav"))
    assert cli.main(base + ["--formant-vtln", "1.15", "--noise-formant"]) == 0
    fs, y = wavfile.read(str(tmp_path / "SA19_modified.wav"))
    _, x = wavfile.read(wav)
    assert fs == 16000 and y.dtype == np.float32 and y.shape == x.shape == plain.shape
    assert np.all(np.isfinite(y)) and np.abs(y).max() > 0.01 and not np.array_equal(y, plain)
