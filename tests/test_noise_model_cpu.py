"""The stochastic component, the parts that need no GPU: the NumPy model of the definition
(tests/noise_model_ref.py) against its own pins (the excitation, scipy's lfilter, silence, the power and the spectrum
of what it resynthesises), the host time maps, and the argument checks of eaQHMNoiseAnalysis, eaQHMNoiseSynthesis,
eaQHMSynthesis(noise=...) and the CLI."""
import numpy as np
import pytest
from scipy.signal import lfilter

import noise_model_ref as N

FS, H, P = 16000, 80, 18


@pytest.fixture(scope="module")
def ar():
    """(e, sigma, refl) of the AR(4) fixture: 2 s at 16 kHz, H = 80, p = 18."""
    e = N.ar_fixture()
    sigma, refl, stop = N.analyse(e, H, P)
    assert not stop.any()
    return e, sigma, refl


def test_excitation_pins():
    x = N.white(7, np.arange(3))
    assert np.allclose(x, [-0.38164095, -1.67389445, 1.38827572], rtol=0, atol=5e-9)
    assert np.array_equal(N.white(7, np.array([-5, -1])), [0.0, 0.0])
    n = np.arange(-100, 5000)
    whole = N.white(123456789, n)
    parts = np.concatenate([N.white(123456789, n[a:b]) for a, b in ((0, 17), (17, 100), (100, 101), (101, len(n)))])
    assert np.array_equal(whole, parts)
    big = N.white(2 ** 64 - 1, np.arange(200000))
    assert abs(big.mean()) < 0.01 and abs(big.var() - 1.0) < 0.01 and np.abs(big).max() <= 3.4641016151377544 / 2


def test_lattice_is_the_all_pole_filter_of_the_stepup():
    rng = np.random.default_rng(1)
    k = np.tanh(rng.normal(size=P) * 0.5)
    x = rng.normal(size=400)
    ref = lfilter([1.0], N.stepup(k), x)
    err = float(np.abs(N.lattice(k, x) - ref).max() / np.abs(ref).max())
    print("lattice vs lfilter: %.3g of the maximum" % err)
    assert err <= 1e-12


def test_synth_runs_the_lattice_of_every_frame(ar):
    """The frame-vectorised synthesis against the per-frame definition: excitation, warm-up from zero state at
    qH - 3H, the 2H kept samples, the cross-fade in increasing q."""
    _, sigma, refl = ar
    L_out = 1000
    tau = N.time_map(H, L_out, 0.8)
    out = N.synth(sigma, refl, H, tau, L_out, 5)
    sg, k = N.frame_parameters(sigma, refl, H, tau)
    v = N.synthesis_window(H)
    ref = np.zeros(L_out)
    for q in range(len(tau)):
        n = np.arange(q * H - 3 * H, q * H + H)
        y = N.lattice(k[q], sg[q] * N.white(5, n))[2 * H:]
        nn = n[2 * H:]
        ok = (nn >= 0) & (nn < L_out)
        ref[nn[ok]] += (v * y)[ok]
    assert np.array_equal(out, ref)


def test_silence_gives_silent_frames_and_exact_zeros(ar):
    e, sigma, refl = ar
    lo, hi = int(0.375 * len(e)), int(0.4375 * len(e))          # 2000 silent samples > 4H
    assert hi - lo > 4 * H
    m = np.arange(len(sigma)) * H
    silent = (m - 2 * H >= lo) & (m + 2 * H <= hi)
    assert silent.sum() >= 10
    assert np.all(sigma[silent] == 0) and np.all(refl[silent] == 0) and np.all(sigma[~silent] > 0)
    out = N.synth(sigma, refl, H, N.time_map(H, len(e), 1.0), len(e), 3)
    ms = np.flatnonzero(silent)
    assert np.all(out[ms[0] * H:ms[-1] * H + 1] == 0.0)
    assert np.abs(out[:lo - 4 * H]).max() > 0


@pytest.mark.parametrize("rho", [1.0, 2.0, 0.5])
def test_resynthesised_noise_keeps_power_and_spectrum(ar, rho):
    """Per 100 ms block the power of the synthesised noise against the input's: +-4 dB.  The bar is about 1.5 x the
    worst figure of a first draw of this fixture (-1.4..+1.0, -0.9..+0.7, -2.5..+1.3 dB at rho 1, 2, 0.5; the statistic
    is a ratio of two 160-sample-bandwidth power estimates); this draw gives -1.5..+1.2, -1.0..+0.7, -3.0..+1.3 dB.  The
    LPC log-spectrum of the re-analysed output against the input's at matching instants: 5 dB rms at worst (first draw
    2.1-2.4 dB mean, 3.3 dB worst; this draw 2.1-2.4 dB mean, 3.5 dB worst).  Fixed seeds: deterministic."""
    e, sigma, refl = ar
    L = len(e)
    Lo = int(np.rint(rho * L))
    y = N.synth(sigma, refl, H, N.time_map(H, Lo, rho), Lo, 1234)
    blk = FS // 10
    nb = L // blk
    bo = int(blk * rho)
    pe = np.array([np.mean(e[i * blk:(i + 1) * blk] ** 2) for i in range(nb)])
    py = np.array([np.mean(y[i * bo:(i + 1) * bo] ** 2) for i in range(nb)])
    good = pe > 1e-8
    ratio = 10 * np.log10(py[good] / pe[good])
    print("rho %g: power ratio %.2f .. %.2f dB" % (rho, ratio.min(), ratio.max()))
    assert good.sum() >= nb - 2 and ratio.min() >= -4.0 and ratio.max() <= 4.0
    s2, k2, _ = N.analyse(y, H, P)
    lo, hi = int(0.375 * L), int(0.4375 * L)
    dist = []
    for m in range(10, len(sigma) - 10, 7):
        if sigma[m] == 0 or lo - 400 < m * H < hi + 400:
            continue
        m2 = min(int(round(m * rho)), len(s2) - 1)
        d = N.lpc_log_spectrum(sigma[m], refl[m]) - N.lpc_log_spectrum(s2[m2], k2[m2])
        dist.append(np.sqrt(np.mean(d ** 2)))
    print("rho %g: log-spectral distance mean %.2f worst %.2f dB" % (rho, np.mean(dist), np.max(dist)))
    assert len(dist) > 30 and np.max(dist) <= 5.0


def test_host_time_maps():
    from eaqhm_amd.model import contour_time_map, noise_time_map, noise_time_map_contour
    for rho, L_out in ((1.0, 32000), (0.5, 16001), (2.0, 63999), (1.37, 81)):
        assert np.array_equal(noise_time_map(H, L_out, rho), N.time_map(H, L_out, rho))
    n, step, length = 200, 15, 199 * 15 + 40
    x = np.arange(n) / (n - 1)
    rho = 1.1 + 0.5 * np.sin(2 * np.pi * 3 * x)
    tm = contour_time_map(rho, np.ones(n), step, length)
    tau = noise_time_map_contour(H, tm, step)
    assert np.array_equal(tau, N.contour_time_map_inverse(H, tm["L_out"], tm["C"], tm["rate"], step))
    assert len(tau) == (tm["L_out"] - 1) // H + 1 and tau[0] == 0 and np.all(np.diff(tau) > 0) and tau[-1] < length
    # the map is the inverse of C: the knots map back to themselves
    one = contour_time_map(np.full(n, 2.0), np.ones(n), step, length)
    assert np.allclose(noise_time_map_contour(1, one, step), np.arange(one["L_out"]) / 2.0, rtol=0, atol=1e-9)


def _noise_model(Nf=26, p=4, hop=8, fs=1600.0):
    return dict(sigma=np.full(Nf, 0.1), refl=np.zeros((Nf, p)), hop=hop, order=p, fs=fs, length=(Nf - 1) * hop + 1)


@pytest.fixture()
def no_device(monkeypatch):
    """Any device work is a failure: the argument checks come first."""
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


@pytest.mark.parametrize("kw", [dict(order=64), dict(order=0), dict(hop=1025), dict(hop=0), dict(hop=2, order=8),
                                dict(hop=2.5), dict(order="x"), dict(fs=-1.0), dict(fs=np.nan), dict(s=np.zeros(0)),
                                dict(s=np.zeros(99)), dict(s=np.zeros((2, 50))), dict(s=np.r_[np.zeros(99), np.nan]),
                                dict(s_recon=np.r_[np.zeros(99), np.inf]), dict(s=["a"] * 100)])
def test_noise_analysis_rejects(kw, no_device):
    from eaqhm_amd import eaQHMNoiseAnalysis
    args = dict(s=np.zeros(100), s_recon=np.zeros(100), fs=16000)
    args.update(kw)
    with pytest.raises(ValueError):
        eaQHMNoiseAnalysis(args.pop("s"), args.pop("s_recon"), args.pop("fs"), **args)


def test_noise_analysis_defaults():
    from eaqhm_amd.model import check_noise_analysis_arguments
    e, fs, hop, order = check_noise_analysis_arguments(np.ones(10), np.arange(10), 16000)
    assert (hop, order, fs) == (80, 18, 16000.0) and e.dtype == np.float64 and np.array_equal(e, 1.0 - np.arange(10))
    assert check_noise_analysis_arguments(np.ones(10), np.ones(10), 48000)[2:] == (240, 50)
    assert check_noise_analysis_arguments(np.ones(10), np.ones(10), 96000)[2:] == (480, 63)
    assert check_noise_analysis_arguments(np.ones(10), np.ones(10), 16000, order=10, hop=3)[2:] == (3, 10)


@pytest.mark.parametrize("edit", [dict(sigma=np.full(25, 0.1)), dict(refl=np.zeros((26, 5))), dict(refl=np.zeros(26)),
                                  dict(hop=0), dict(order=64), dict(length=300), dict(fs=0.0),
                                  dict(sigma=np.r_[np.full(25, 0.1), -1.0]), dict(sigma=np.r_[np.full(25, 0.1), np.nan]),
                                  dict(refl=np.full((26, 4), 1.0)), dict(refl=np.full((26, 4), np.nan)),
                                  dict(tau=np.zeros(25)), dict(tau=np.r_[np.zeros(25), -1.0]),
                                  dict(tau=np.r_[np.zeros(25), np.nan]), dict(tau=np.zeros((2, 13))), dict(L_out=0),
                                  dict(L_out=201.5), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5)])
def test_noise_synthesis_rejects(edit, no_device):
    from eaqhm_amd import eaQHMNoiseSynthesis
    nz = _noise_model()
    args = dict(tau=np.arange(26) * 8.0, L_out=201, seed=0)
    for k, v in edit.items():
        (args if k in args else nz)[k] = v
    with pytest.raises(ValueError):
        eaQHMNoiseSynthesis(nz, args["tau"], args["L_out"], args["seed"])
    with pytest.raises(ValueError):
        eaQHMNoiseSynthesis("model", args["tau"], args["L_out"])


def test_noise_synthesis_checks_pass_a_good_call():
    from eaqhm_amd.model import check_noise_synthesis_arguments
    nz, tau, L_out, seed = check_noise_synthesis_arguments(_noise_model(), list(range(0, 208, 8)), 201.0, 2 ** 64 - 1)
    assert tau.dtype == np.float64 and len(tau) == 26 and L_out == 201 and seed == 2 ** 64 - 1
    assert nz["refl"].flags["C_CONTIGUOUS"] and nz["refl"].shape == (26, 4) and nz["hop"] == 8


def _arrays_model(n=8, K=2, step=15):
    ti = np.arange(n) * step
    return dict(ti=ti, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=np.full((n, K), 0.1),
                frange=np.tile([200.0, 400.0], (n, 1))[:, :K], pk=np.zeros((n, K)))


@pytest.mark.parametrize("kw", [dict(noise="x"), dict(noise=dict(sigma=np.zeros(3))),
                                dict(noise=_noise_model(fs=16000.0)),                 # another length (201, not 200)
                                dict(noise=dict(_noise_model(), length=200)),         # sigma does not fit the length
                                dict(noise=_noise_model()),                           # another fs
                                dict(noise=dict(_noise_model(fs=16000.0), refl=np.ones((26, 4)))),
                                dict(noise=None, noise_seed=0, time_scale=9.0)])
def test_synthesis_rejects_a_bad_noise_model(kw, no_device):
    from eaqhm_amd.model import eaQHMSynthesis
    with pytest.raises(ValueError):
        eaQHMSynthesis(_arrays_model(), 16000, 200, **kw)


def test_synthesis_rejects_a_bad_noise_seed(no_device):
    from eaqhm_amd.model import eaQHMSynthesis
    nz = _noise_model(Nf=25, fs=16000.0)
    nz["length"], nz["sigma"], nz["refl"] = 200, np.full(25, 0.1), np.zeros((25, 4))
    with pytest.raises(ValueError):
        eaQHMSynthesis(_arrays_model(), 16000, 200, noise=nz, noise_seed=-3)
    with pytest.raises(AssertionError):        # a good model and seed pass the checks and reach the device
        eaQHMSynthesis(_arrays_model(), 16000, 200, noise=nz, noise_seed=3)


def test_binding_and_exports():
    import eaqhm_amd
    from eaqhm_amd import hip
    assert hip.ABI_VERSION == 6
    names = {n for n, _, _ in hip.SYMBOLS}
    assert {"eaqhm_noise_analyse", "eaqhm_noise_synth"} <= names
    for name in ("eaQHMNoiseAnalysis", "eaQHMNoiseSynthesis", "noise_time_map", "noise_time_map_contour", "read_signal"):
        assert callable(getattr(eaqhm_amd, name))


def test_cli_noise_flags(tmp_path):
    from eaqhm_amd import cli
    a = cli.parser().parse_args(["x.wav", "--noise", "--noise-seed", "12", "--time-scale", "1.5"])
    assert a.noise and a.noise_seed == 12 and a.time_scale == 1.5
    a = cli.parser().parse_args(["x.wav"])
    assert not a.noise and a.noise_seed is None
    missing = str(tmp_path / "missing.wav")
    with pytest.raises(SystemExit):
        cli.main([missing, "--noise-seed", "3"])                 # needs --noise
    with pytest.raises(SystemExit):
        cli.main([missing, "--noise", "--noise-seed", "x"])
    with pytest.raises(ValueError):
        cli.main([missing, "--noise", "--noise-seed", "-1"])     # rejected before the analysis
    with pytest.raises(FileNotFoundError):
        cli.main([missing, "--noise", "--noise-seed", "4"])      # accepted: the analysis starts
