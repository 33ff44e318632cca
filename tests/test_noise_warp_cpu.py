"""The formant warp of the noise model, the parts that need no GPU: the NumPy model of the definition
(tests/noise_warp_ref.py) against the exact warped spectrum, its pass-throughs, the host contour, the argument checks of
eaQHMNoiseWarp, noise_envelope, noise_formant_contour and eaQHMSynthesis(noise_formant=...), the binding and the CLI."""
import numpy as np
import pytest

import noise_model_ref as N
import noise_warp_ref as W

FS, H, P = 16000, 80, 18


@pytest.fixture(scope="module")
def ar():
    """(sigma, refl) of the AR(4) fixture: 2 s at 16 kHz, H = 80, p = 18 (400 frames, 22 silent)."""
    sigma, refl, stop = N.analyse(N.ar_fixture(), H, P)
    assert not stop.any()
    return sigma, refl


@pytest.mark.parametrize("alpha", [0.85, 1.2, 0.5, 2.0])
def test_refit_represents_the_warped_spectrum(ar, alpha):
    """Every 7th non-silent frame, 200 frequencies in [0.02, 0.98 pi min(alpha, 1)] rad: the rms log-spectral distance
    between the refit's spectrum and the exact warped spectrum of the input stays under 3 dB (about 1.5 x the worst
    value of the prototype, 2.02 dB at alpha = 0.5).  No frame stops its recursion early, none is excluded.  This
    model: 0.65 / 1.27, 0.11 / 0.39, 1.31 / 2.02, 0.02 / 0.07 dB (mean / worst) at alpha 0.85, 1.2, 0.5, 2."""
    sigma, refl = ar
    frames = np.flatnonzero(sigma > 0)[::7]
    assert len(frames) == 54
    w = np.linspace(0.02, 0.98 * np.pi * min(alpha, 1.0), 200)
    fnorm = w / (2 * np.pi)
    s2, k2, stop = W.warp(sigma[frames], refl[frames], alpha)
    assert not stop.any() and np.all(s2 > 0) and np.abs(k2).max() < 1
    exact = W.envelope(sigma[frames], refl[frames], alpha, fnorm)
    refit = W.envelope(s2, k2, 1.0, fnorm)
    dist = np.sqrt(np.mean((W.DB * (refit - exact)) ** 2, axis=1))
    print("alpha %g: rms distance mean %.2f worst %.2f dB, max|k'| %.3f" % (alpha, dist.mean(), dist.max(),
                                                                            np.abs(k2).max()))
    assert dist.max() < 3.0


def test_grid_size_hardly_matters(ar, monkeypatch):
    """The refit on a 512-point grid is the 1024-point one to well under the distances above."""
    sigma, refl = ar
    frames = np.flatnonzero(sigma > 0)[::40]
    a = W.warp(sigma[frames], refl[frames], 0.85)
    monkeypatch.setattr(W, "M", 512)
    monkeypatch.setattr(W, "_TABLES", {})
    b = W.warp(sigma[frames], refl[frames], 0.85)
    assert np.abs(a[1] - b[1]).max() < 1e-3 and np.abs(a[0] / b[0] - 1).max() < 1e-3


def test_unit_scale_and_silence_pass_through(ar):
    sigma, refl = ar
    s2, k2, stop = W.warp(sigma, refl, 1.0)
    assert np.array_equal(s2, sigma) and np.array_equal(k2, refl) and not stop.any()
    silent = sigma == 0
    assert silent.sum() == 22
    s2, k2, _ = W.warp(sigma[silent], np.full((22, P), 0.3), 1.2)
    assert np.all(s2 == 0) and np.all(k2 == 0)
    # a contour that is 1 on a stretch returns the input frames there, and warps the others
    alpha = np.where(np.arange(len(sigma)) < 100, 1.0, 1.2)
    s2, k2, _ = W.warp(sigma[90:110], refl[90:110], alpha[90:110])
    assert np.array_equal(s2[:10], sigma[90:100]) and np.array_equal(k2[:10], refl[90:100])
    assert np.all(s2[10:] != sigma[100:110])
    # the refit at alpha = 1, were it run, is close but not the input: why alpha == 1 is a pass-through
    k1, E, _ = W.levinson(W.warped_autocorrelation(sigma[5], refl[5], 1.0), P)
    assert 0 < np.abs(k1 - refl[5]).max() < 1e-6


def test_warp_moves_a_spectral_peak():
    """One resonance at 0.5 rad: the refit's spectrum peaks at 0.5 alpha."""
    k = N.analyse(N.ar_fixture(0.5), H, 4)[1][40]
    w = np.linspace(0.05, 3.0, 2000)
    peak0 = w[np.argmax(W.envelope([1.0], [k], 1.0, w / (2 * np.pi))[0])]
    for alpha in (0.85, 1.2):
        s2, k2, _ = W.warp([1.0], [k], alpha)
        peak = w[np.argmax(W.envelope(s2, k2, 1.0, w / (2 * np.pi))[0])]
        assert abs(peak - alpha * peak0) < 0.02, (alpha, peak, peak0)


def _noise_model(Nf=26, p=4, hop=8, fs=1600.0):
    return dict(sigma=np.full(Nf, 0.1), refl=np.zeros((Nf, p)), hop=hop, order=p, fs=fs, length=(Nf - 1) * hop + 1)


def _arrays_model(n=8, K=2, step=15):
    ti = np.arange(n) * step
    return dict(ti=ti, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=np.full((n, K), 0.1),
                frange=np.tile([200.0, 400.0], (n, 1))[:, :K], pk=np.zeros((n, K)))


def test_noise_formant_contour_is_np_interp():
    from eaqhm_amd import noise_formant_contour
    det = _arrays_model(n=12)                      # instants 0, 15, .., 165
    nz = _noise_model(Nf=26, hop=8)                # frames 0, 8, .., 200: the last ones lie past the last instant
    alpha = np.linspace(0.8, 1.3, 12) ** 2
    got = noise_formant_contour(nz, det, alpha)
    assert got.dtype == np.float64 and got.shape == (26,)
    assert np.array_equal(got, np.interp(np.arange(26) * 8.0, det["ti"].astype(np.float64), alpha))
    assert np.array_equal(got, W.contour(8, 26, det["ti"], alpha))
    assert got[0] == alpha[0] and np.all(got[21:] == alpha[-1])
    assert np.array_equal(noise_formant_contour(nz, det, 1.18), np.full(26, 1.18))
    for bad in (np.ones(11), 5.0, np.full(12, np.nan), "x", np.ones((12, 1))):
        with pytest.raises(ValueError):
            noise_formant_contour(nz, det, bad)
    with pytest.raises(ValueError):
        noise_formant_contour("model", det, 1.0)


@pytest.fixture()
def no_device(monkeypatch):
    """Any device work is a failure: the argument checks come first."""
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


@pytest.mark.parametrize("alpha", [0.2, 4.5, np.nan, np.inf, "x", None, np.ones(25), np.ones((26, 1)),
                                   np.r_[np.ones(25), 0.1], np.r_[np.ones(25), np.nan], ["a"] * 26])
def test_noise_warp_rejects(alpha, no_device):
    from eaqhm_amd import eaQHMNoiseWarp
    with pytest.raises(ValueError):
        eaQHMNoiseWarp(_noise_model(), alpha)


def test_noise_warp_rejects_a_bad_model(no_device):
    from eaqhm_amd import eaQHMNoiseWarp, noise_envelope
    for bad in ("model", dict(sigma=np.zeros(3)), dict(_noise_model(), order=64),
                dict(_noise_model(), refl=np.ones((26, 4)))):
        with pytest.raises(ValueError):
            eaQHMNoiseWarp(bad, 1.2)
        with pytest.raises(ValueError):
            noise_envelope(bad, 1600.0, [100.0])
    with pytest.raises(AssertionError):        # a good call passes the checks and reaches the device
        eaQHMNoiseWarp(_noise_model(), np.full(26, 1.2))


@pytest.mark.parametrize("kw", [dict(fs=16000.0), dict(fs=0.0), dict(fs=np.nan), dict(freqs=[]), dict(freqs=[-1.0]),
                                dict(freqs=[np.nan]), dict(freqs=[[1.0, 2.0]]), dict(freqs=["a"]),
                                dict(formant_scale=5.0), dict(formant_scale=np.ones(3))])
def test_noise_envelope_rejects(kw, no_device):
    from eaqhm_amd import noise_envelope
    args = dict(fs=1600.0, freqs=[0.0, 100.0, 800.0], formant_scale=1.0)
    args.update(kw)
    with pytest.raises(ValueError):
        noise_envelope(_noise_model(), args["fs"], args["freqs"], args["formant_scale"])


def test_checks_pass_good_calls():
    from eaqhm_amd.model import check_noise_envelope_arguments, check_noise_warp_arguments
    nz, alpha = check_noise_warp_arguments(_noise_model(), 2)
    assert alpha.dtype == np.float64 and np.array_equal(alpha, np.full(26, 2.0)) and nz["order"] == 4
    nz, alpha = check_noise_warp_arguments(_noise_model(), list(np.linspace(0.25, 4.0, 26)))
    assert alpha[0] == 0.25 and alpha[-1] == 4.0 and alpha.flags["C_CONTIGUOUS"]
    nz, alpha, fnorm = check_noise_envelope_arguments(_noise_model(), 1600, [0, 400, 800, 1000], 1.0)
    assert np.array_equal(fnorm, [0.0, 0.25, 0.5, 0.625]) and len(alpha) == 26


def test_synthesis_noise_formant_checks(no_device):
    from eaqhm_amd.model import eaQHMSynthesis
    nz = _noise_model(Nf=25, fs=16000.0)
    nz["length"] = 200
    det = _arrays_model()
    for kw in (dict(noise_formant=True),                                          # needs noise=
               dict(noise=nz, noise_formant=True, preserve_envelope=False),       # needs the envelope
               dict(noise=nz, noise_formant=1), dict(noise=nz, noise_formant="yes"), dict(noise=nz, noise_formant=None)):
        with pytest.raises(ValueError):
            eaQHMSynthesis(det, 16000, 200, formant_scale=1.0, **kw)
    with pytest.raises(ValueError):
        eaQHMSynthesis(det, 16000, 200, formant_scale=9.0, noise=nz, noise_formant=True)
    with pytest.raises(AssertionError):        # a good call passes the checks and reaches the device
        eaQHMSynthesis(det, 16000, 200, formant_scale=1.2, noise=nz, noise_formant=True)


def test_binding_and_exports():
    import eaqhm_amd
    from eaqhm_amd import hip
    assert hip.ABI_VERSION == 6
    sym = {n: a for n, _, a in hip.SYMBOLS}
    assert len(sym["eaqhm_noise_warp"]) == 8 and len(sym["eaqhm_noise_envelope"]) == 9
    for name in ("eaQHMNoiseWarp", "noise_formant_contour", "noise_envelope"):
        assert callable(getattr(eaqhm_amd, name))
    assert callable(hip.Context.noise_warp) and callable(hip.Context.noise_envelope)


def test_cli_noise_formant_flag(tmp_path):
    from eaqhm_amd import cli
    a = cli.parser().parse_args(["x.wav", "--noise", "--noise-formant", "--formant-scale", "1.18"])
    assert a.noise and a.noise_formant and a.formant_scale == 1.18
    assert not cli.parser().parse_args(["x.wav", "--noise"]).noise_formant
    missing = str(tmp_path / "missing.wav")
    with pytest.raises(SystemExit):
        cli.main([missing, "--noise-formant", "--formant-scale", "1.2"])           # needs --noise
    with pytest.raises(SystemExit):
        cli.main([missing, "--noise", "--noise-formant"])                          # needs a formant scale flag
    with pytest.raises(SystemExit):
        cli.main([missing, "--noise", "--noise-formant", "--time-scale", "1.5"])
    with pytest.raises(ValueError):
        cli.main([missing, "--noise", "--noise-formant", "--formant-scale", "9"])  # rejected before the analysis
    with pytest.raises(FileNotFoundError):
        cli.main([missing, "--noise", "--noise-formant", "--formant-scale", "1.2"])    # accepted: the analysis starts
    curve = tmp_path / "alpha.txt"
    curve.write_text("0 1.0\n1 1.2\n")
    with pytest.raises(FileNotFoundError):
        cli.main([missing, "--noise", "--noise-formant", "--formant-scale-curve", str(curve)])
