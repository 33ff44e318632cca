"""Pitch-synchronous modulation of the noise, the parts that need no GPU: the NumPy model of the
definition (tests/noise_modulation_ref.py) against a constructed ground truth and its exact properties, the host
functions model_phase and noise_fundamental, the argument checks, the binding and the CLI flag.

Bars of the ground-truth tests.  Fixture: a one-slot model gliding 180 -> 300 Hz over 2 s at 16 kHz (step 15, ph = 2 pi
integral f0), residual e = g_true(Theta(n)) x white Gaussian noise with c_1 = 0.4 e^{0.9 i}; H = 80, M = 2; c_1 averaged
over all 400 frames (all voiced, none left out).  The NumPy model alone, seeds 11, 12, 13, 14:
  analysis    |mean c_1| - 0.4: -0.0074, -0.0080, +0.0068, -0.0052;  angle error: +0.0182, +0.0035, -0.0126, -0.0085 rad
              bars (twice the worst): 0.016 in modulus, 0.0364 rad
              unmodulated residual, |mean c_1|: 0.0077, 0.0070, 0.0140, 0.0047 (bar 0.016); the mean of |c_1| over the
              frames, the chance value of one frame, is 0.097 - 0.101
  synthesis   (LPC model of that residual, p = 18; re-analysed against theta + nu (n' - qH) of the nearest output frame)
              unit scales:          modulus -0.0111, +0.0002, +0.0052, -0.0068;  angle +0.0201, +0.0022, -0.0152, -0.0186
              rho 1.5, beta 1.3:    modulus -0.0054, -0.0059, +0.0053, -0.0059;  angle +0.0197, +0.0101, -0.0168, -0.0059
              bars (twice the worst): 0.0222 in modulus, 0.0402 rad
              at beta 1.3 against the old pitch (the model's phase at tau, without the advance): |mean c_1| 0.0031,
              0.0055, 0.0028, 0.0079: under the modulus bar, while the new pitch gives 0.39 - 0.41"""
import os

import numpy as np
import pytest

import noise_model_ref as N
import noise_modulation_ref as R

FS, H, P, STEP = 16000, 80, 18, 15
C1 = 0.4 * np.exp(0.9j)
SEEDS = (11, 12, 13, 14)
BAR_MOD, BAR_ANG = 0.016, 0.0364            # analysis: twice the worst of the four seeds (docstring)
BAR_SYN_MOD, BAR_SYN_ANG = 0.0222, 0.0402   # synthesis round trip: twice the worst


@pytest.fixture(scope="module")
def glide():
    det, rec, L = R.glide_model(FS, 2.0, STEP)
    return det, rec, L, R.model_f0(rec), R.model_phase(rec, STEP, FS), R.voiced_flags(rec)


def _c1(mod):
    return complex((mod[:, 0] + 1j * mod[:, 1]).mean())


def _structs(det):
    """The det_format="structs" form of an arrays model: shape-(1,) cells, the int 0 in inactive cells."""
    from eaqhm_amd.structs import Deterministic
    out = []
    for i, ti in enumerate(det["ti"]):
        x = Deterministic(ti=int(ti), isSpeech=True, isVoiced=True, a0=float(det["a0"][i]))
        act = det["amplitudes"][i] != 0
        for name in ("amplitudes", "frange", "pk"):
            setattr(x, name, [np.array([v]) if a else 0 for v, a in zip(det[name][i], act)])
        out.append(x)
    return out


def _hand_model():
    """12 instants, 2 slots; slot 0 inactive at 0, 1 (before the first anchored instant), 5, 6 (a gap) and 11."""
    n = 12
    ti = np.arange(n) * STEP
    f = 200.0 + 3.0 * np.arange(n)
    am = np.full((n, 2), 0.1)
    am[[0, 1, 5, 6, 11], 0] = 0.0
    ph = np.column_stack((0.3 + 1.7 * np.arange(n), -2.0 + 0.9 * np.arange(n)))
    return dict(ti=ti, a0=np.zeros(n), amplitudes=am, frange=np.column_stack((f, 2 * f + 1.0)), pk=ph)


def test_model_phase_anchors_and_bridges():
    from eaqhm_amd import model_f0, model_phase, unpack_model
    det = _hand_model()
    th = model_phase(det, FS)
    f0 = model_f0(det, FS)
    assert th.shape == (12,) and th.dtype == np.float64 and np.all((th >= 0) & (th < 1))
    for i in (2, 3, 4, 7, 8, 9, 10):
        x = det["pk"][i, 0] / (2 * np.pi)
        assert th[i] == x - np.floor(x)

    def step(a, i, j):
        return (STEP / FS) * (f0[i] + f0[j]) / 2

    for i in (5, 6, 11):                                     # forwards from the previous instant
        x = th[i - 1] + step(th, i - 1, i)
        assert th[i] == x - np.floor(x)
    for i in (1, 0):                                         # backwards from the first anchored one
        x = th[i + 1] - step(th, i, i + 1)
        assert th[i] == x - np.floor(x)
    assert np.array_equal(th, R.model_phase(unpack_model(det)["records"], STEP, FS))
    assert np.array_equal(model_phase(_structs(det), FS), th)
    # a given f0 drives the bridges and leaves the anchors; a model without slot 0 starts from 0
    th2 = model_phase(det, FS, f0=np.full(12, 100.0))
    assert np.array_equal(th2[[2, 3, 4, 7]], th[[2, 3, 4, 7]]) and th2[5] != th[5]
    none = dict(det, amplitudes=np.column_stack((np.zeros(12), det["amplitudes"][:, 1])))
    th3 = model_phase(none, FS)
    assert th3[0] == 0.0 and np.all(np.diff(th3) != 0)
    for bad in (np.zeros(12), np.full(11, 100.0), np.r_[np.full(11, 100.0), np.nan]):
        with pytest.raises(ValueError):
            model_phase(det, FS, f0=bad)


def test_analysis_recovers_a_known_modulation(glide):
    _, rec, L, f0, th, vo = glide
    assert vo.all()
    for seed in SEEDS:
        mod = R.analyse(R.modulated_residual(rec, STEP, FS, L, C1, seed), H, 2, th, f0, vo, 0.0, STEP, FS)
        assert mod.shape == ((L - 1) // H + 1, 4)
        c = _c1(mod)
        flat = _c1(R.analyse(0.01 * np.random.default_rng(seed).normal(size=L), H, 2, th, f0, vo, 0.0, STEP, FS))
        print("seed %d: |c_1| - 0.4 = %+.4f, angle %+.4f rad; unmodulated |mean c_1| %.4f"
              % (seed, abs(c) - 0.4, np.angle(c * np.conj(C1)), abs(flat)))
        assert abs(abs(c) - abs(C1)) <= BAR_MOD, (seed, abs(c))
        assert abs(np.angle(c * np.conj(C1))) <= BAR_ANG, (seed, np.angle(c * np.conj(C1)))
        assert abs(flat) <= BAR_MOD, (seed, abs(flat))


@pytest.mark.parametrize("rho, beta", [(1.0, 1.0), (1.5, 1.3)])
def test_synthesis_plays_the_modulation_at_the_output_pitch(glide, rho, beta):
    _, rec, L, f0, th, vo = glide
    n = len(rec)
    for seed in SEEDS:
        e = R.modulated_residual(rec, STEP, FS, L, C1, seed)
        mod = R.analyse(e, H, 2, th, f0, vo, 0.0, STEP, FS)
        sg, k, _ = N.analyse(e, H, P)
        Lo = int(np.rint(rho * L))
        tau = N.time_map(H, Lo, rho)
        thq, nuq = R.fundamental(rec, STEP, FS, tau, np.full(n - 1, beta * rho), np.full(n, rho), beta * rho)
        y = R.synth_mod(sg, k, H, tau, Lo, seed + 100, mod, thq, nuq)
        c = _c1(R.analyse_phase(y, H, 2, R.output_phase(thq, nuq, H, Lo)))
        print("rho %g beta %g seed %d: |c_1| - 0.4 = %+.4f, angle %+.4f rad"
              % (rho, beta, seed, abs(c) - 0.4, np.angle(c * np.conj(C1))))
        assert abs(abs(c) - abs(C1)) <= BAR_SYN_MOD, (seed, abs(c))
        assert abs(np.angle(c * np.conj(C1))) <= BAR_SYN_ANG, (seed, np.angle(c * np.conj(C1)))
        if beta != 1.0:      # the envelope follows the new pitch: against the old one nothing is left
            old = _c1(R.analyse_phase(y, H, 2, R.phase_at(np.arange(Lo) / rho, th, f0, 0.0, STEP, FS)))
            print("   against the old pitch |mean c_1| %.4f" % abs(old))
            assert abs(old) <= BAR_SYN_MOD, (seed, abs(old))


def test_exact_properties_of_the_model(glide):
    _, rec, L, f0, th, vo = glide
    L = 8000
    e = R.modulated_residual(rec, STEP, FS, L, C1, 5)
    e[3000:3500] = 0.0                                         # 500 silent samples > 4H
    unv = vo.copy()
    unv[(np.arange(len(vo)) * STEP >= 5000) & (np.arange(len(vo)) * STEP < 6000)] = False
    mod = R.analyse(e, H, 3, th, f0, unv, 0.0, STEP, FS)
    m = np.arange(len(mod)) * H
    silent = (m - 2 * H >= 3000) & (m + 2 * H <= 3500)
    unvoiced = ~unv[R.nearest(m, 0.0, STEP, len(unv))]
    assert silent.sum() >= 2 and unvoiced.sum() >= 10
    assert np.all(mod[silent | unvoiced] == 0.0) and np.all(np.abs(mod[~(silent | unvoiced)]).sum(axis=1) > 0)
    # the stored coefficients do not depend on M
    assert np.array_equal(R.analyse(e, H, 1, th, f0, unv, 0.0, STEP, FS), mod[:, :2])
    sg, k, _ = N.analyse(e, H, P)
    Lo = 5003
    tau = N.time_map(H, Lo, 0.625)
    n = len(rec)
    thq, nuq = R.fundamental(rec, STEP, FS, tau, np.full(n - 1, 0.75), np.full(n, 0.625), 0.75)
    y = R.frames(sg, k, H, tau, Lo, 9)
    plain = N.synth(sg, k, H, tau, Lo, 9)
    assert np.array_equal(R.synth_mod(sg, k, H, tau, Lo, 9, np.zeros_like(mod), thq, nuq, y=y), plain)
    whole = R.synth_mod(sg, k, H, tau, Lo, 9, mod, thq, nuq, y=y)
    assert not np.array_equal(whole, plain)
    parts = sum(R.synth_mod(sg, k, H, tau, Lo, 9, mod, thq, nuq, t_lo=a, t_hi=b, y=y)
                for a, b in ((0, 1337), (1337, 80 * 40), (80 * 40, Lo)))
    assert np.array_equal(parts, whole)
    # a mod that would drive g^2 negative: the floor is reached and held
    deep = np.zeros((1, 2))
    deep[0, 0] = 0.9                                           # g^2 = 1 + 1.8 cos: negative around theta = 1/2
    d = np.arange(-H, H)
    g = R.gain_of(deep[0], 0.5, 1e-3, d)
    g2 = 1 + 1.8 * np.cos(2 * np.pi * (0.5 + 1e-3 * d))
    assert g2.min() < 0 and np.all(g[g2 <= R.FLOOR] == np.sqrt(R.FLOOR)) and g.min() == 0.1
    assert np.allclose(g[g2 > R.FLOOR], np.sqrt(g2[g2 > R.FLOOR]), rtol=1e-12, atol=0)


def _circ(a, b):
    d = np.abs(a - b)
    return np.minimum(d, 1 - d)


@pytest.mark.parametrize("path", ["scalar", "contour"])
def test_noise_fundamental_matches_the_model_and_its_own_rate(glide, path):
    """theta_{q+1} - theta_q against nu_q H.  Bound: the derivative of Theta(tau(n')) + s(n') is (g/rho)(F + (f0_i - F)
    / g) / fs with i the nearest instant, so it is off nu(n') by at most dF / (2 rho fs), dF = max |f0_{i+1} - f0_i|;
    nu(n') moves over a frame (H / rho input samples, at most H / (rho D) + 1 intervals) by at most that many steps of
    (g/rho) dF / fs and of F_max |delta (g/rho)| / fs.  Times H, plus 1e-9 for rounding (the trapezoid steps of Theta
    are exact for a linear f0)."""
    from eaqhm_amd import contour_time_map, noise_fundamental, noise_time_map, noise_time_map_contour
    det, rec, L, f0, th, vo = glide
    n = len(rec)
    if path == "scalar":
        rho, beta = 1.5, 1.3
        Lo = int(np.rint(rho * L))
        tau = noise_time_map(H, Lo, rho)
        theta, nu = noise_fundamental(det, FS, tau, time_scale=rho, pitch_scale=beta)
        gain, rate, g_last = np.full(n - 1, beta * rho), np.full(n, rho), beta * rho
    else:
        x = np.arange(n) / (n - 1)
        rho_c, beta_c = 1.1 + 0.5 * np.sin(2 * np.pi * 3 * x), 0.8 + 0.5 * x
        tm = contour_time_map(rho_c, beta_c, STEP, L)
        tau = noise_time_map_contour(H, tm, STEP)
        theta, nu = noise_fundamental(det, FS, tau, time_map=tm, pitch_scale=beta_c)
        gain, rate, g_last = tm["gain"], tm["rate"], tm["rate"][-1] * beta_c[-1]
    assert theta.shape == nu.shape == tau.shape and np.all((theta >= 0) & (theta < 1)) and np.all(nu > 0)
    ref_t, ref_n = R.fundamental(rec, STEP, FS, tau, gain, rate, g_last)
    assert _circ(theta, ref_t).max() <= 1e-11 and np.abs(nu - ref_n).max() <= 1e-15
    ratio = gain / rate[:-1]
    steps = H / (rate.min() * STEP) + 1
    dF = np.abs(np.diff(f0)).max()
    bound = H * (steps * (ratio.max() * dF + f0.max() * np.abs(np.diff(ratio)).max()) / FS
                 + dF / (2 * rate.min() * FS)) + 1e-9
    inside = tau[1:] <= (n - 1) * STEP
    dev = _circ((theta[1:] - theta[:-1]) % 1.0, (nu[:-1] * H) % 1.0)[inside]
    print("%s: finite difference of theta against nu H: %.3g cycles at most, bound %.3g" % (path, dev.max(), bound))
    assert inside.sum() > 100 and dev.max() <= bound
    assert bound < 0.05                                     # the bound says something: nu H is 0.9 - 2 cycles


def test_unit_scales_give_the_analysed_phase(glide):
    from eaqhm_amd import noise_fundamental, noise_time_map
    det, rec, L, f0, th, vo = glide
    tau = noise_time_map(H, L, 1.0)
    theta, nu = noise_fundamental(det, FS, tau)
    ref = R.phase_at(tau, th, f0, 0.0, STEP, FS)
    assert np.array_equal(theta, R.frac(ref))
    assert np.allclose(nu, np.interp(tau, np.arange(len(f0)) * STEP, f0) / FS, rtol=1e-15, atol=0)


@pytest.fixture()
def no_device(monkeypatch):
    """Any device work is a failure: the argument checks come first."""
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


def _noise_model(Nf=26, p=4, hop=8, fs=16000.0, M=None):
    nz = dict(sigma=np.full(Nf, 0.1), refl=np.zeros((Nf, p)), hop=hop, order=p, fs=fs, length=(Nf - 1) * hop + 1)
    if M:
        nz.update(mod=np.zeros((Nf, 2 * M)), mod_harmonics=M)
    return nz


def _arrays_model(n=14, K=2, step=15):
    ti = np.arange(n) * step
    return dict(ti=ti, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=np.full((n, K), 0.1),
                frange=np.tile([200.0, 400.0], (n, 1))[:, :K], pk=np.zeros((n, K)))


def test_check_noise_model_takes_and_validates_the_two_keys():
    from eaqhm_amd.model import check_noise_model
    plain = check_noise_model(_noise_model())
    assert "mod" not in plain and "mod_harmonics" not in plain
    nz = check_noise_model(dict(_noise_model(M=3), mod=[[0.1] * 6] * 26, mod_harmonics=3.0))
    assert nz["mod"].shape == (26, 6) and nz["mod"].dtype == np.float64 and nz["mod"].flags["C_CONTIGUOUS"]
    assert nz["mod_harmonics"] == 3 and isinstance(nz["mod_harmonics"], int)
    for edit in (dict(mod_harmonics=0), dict(mod_harmonics=9), dict(mod_harmonics=2.5), dict(mod_harmonics=2),
                 dict(mod=np.zeros((25, 6))), dict(mod=np.zeros(26 * 6)), dict(mod=np.full((26, 6), np.nan)),
                 dict(mod=np.full((26, 6), np.inf)), dict(mod=[["a"] * 6] * 26)):
        with pytest.raises(ValueError):
            check_noise_model(dict(_noise_model(M=3), **edit))
    for key in ("mod", "mod_harmonics"):
        half = _noise_model(M=3)
        del half[key]
        with pytest.raises(ValueError):
            check_noise_model(half)


@pytest.mark.parametrize("kw", [dict(harmonics=0), dict(harmonics=9), dict(harmonics=1.5), dict(harmonics="x"),
                                dict(harmonics=True), dict(s=np.zeros(200)), dict(s_recon=np.zeros(200)),
                                dict(s=np.r_[np.zeros(200), np.nan]), dict(noise="x"), dict(noise=_noise_model(Nf=25)),
                                dict(det=_arrays_model(n=15)), dict(det=dict(_arrays_model(), ti=np.arange(14) * 15 + 1)),
                                dict(f0=np.zeros(14)), dict(f0=np.full(13, 100.0)), dict(f0="x")])
def test_noise_modulation_rejects(kw, no_device):
    from eaqhm_amd import eaQHMNoiseModulation
    args = dict(s=np.zeros(201), s_recon=np.zeros(201), noise=_noise_model(), det=_arrays_model(), harmonics=2, f0=None)
    args.update(kw)
    with pytest.raises(ValueError):
        eaQHMNoiseModulation(args["s"], args["s_recon"], args["noise"], args["det"], args["harmonics"], args["f0"])


def test_noise_modulation_good_call_reaches_the_device(no_device):
    from eaqhm_amd import eaQHMNoiseModulation
    with pytest.raises(AssertionError):
        eaQHMNoiseModulation(np.zeros(201), np.zeros(201), _noise_model(), _arrays_model(), 8, np.full(14, 150.0))


@pytest.mark.parametrize("fund", [(np.zeros(25), np.zeros(26)), (np.zeros(26), np.zeros(27)), np.zeros(26),
                                  (np.zeros(26),), (np.r_[np.zeros(25), np.nan], np.zeros(26)),
                                  (np.zeros(26), np.r_[np.zeros(25), np.inf]), (np.zeros((2, 13)), np.zeros(26)), "xy"])
def test_noise_synthesis_rejects_a_bad_fundamental(fund, no_device):
    from eaqhm_amd import eaQHMNoiseSynthesis
    with pytest.raises(ValueError):
        eaQHMNoiseSynthesis(_noise_model(M=2), np.arange(26) * 8.0, 201, 0, fund)


def test_noise_synthesis_fundamental_needs_mod(no_device):
    from eaqhm_amd import eaQHMNoiseSynthesis
    good = (np.zeros(26), np.zeros(26))
    with pytest.raises(ValueError, match="mod"):
        eaQHMNoiseSynthesis(_noise_model(), np.arange(26) * 8.0, 201, 0, good)
    with pytest.raises(ValueError, match="mod"):
        eaQHMNoiseSynthesis(_noise_model(), np.arange(26) * 8.0, 201, fundamental=good)
    with pytest.raises(AssertionError):          # a good call passes the checks and reaches the device
        eaQHMNoiseSynthesis(_noise_model(M=2), np.arange(26) * 8.0, 201, 0, good)
    with pytest.raises(AssertionError):          # and so does a mod-carrying model without fundamental
        eaQHMNoiseSynthesis(_noise_model(M=2), np.arange(26) * 8.0, 201)


@pytest.mark.parametrize("kw", [dict(noise_modulation=True), dict(noise=_noise_model(), noise_modulation=True),
                                dict(noise=_noise_model(M=2), noise_modulation=1),
                                dict(noise=_noise_model(M=2), noise_modulation="yes"),
                                dict(noise=dict(_noise_model(M=2), mod_harmonics=9), noise_modulation=True)])
def test_synthesis_rejects_bad_noise_modulation(kw, no_device):
    from eaqhm_amd import eaQHMSynthesis
    with pytest.raises(ValueError):
        eaQHMSynthesis(_arrays_model(), 16000, 201, **kw)


def test_synthesis_good_noise_modulation_reaches_the_device(no_device):
    from eaqhm_amd import eaQHMSynthesis
    for kw in (dict(noise_modulation=True), dict(noise_modulation=False), dict(noise_modulation=True, phase="shape")):
        with pytest.raises(AssertionError):
            eaQHMSynthesis(_arrays_model(), 16000, 201, noise=_noise_model(M=2), **kw)


@pytest.mark.parametrize("kw", [dict(tau=np.r_[np.zeros(3), -1.0]), dict(tau=np.zeros((2, 2))), dict(tau=[]),
                                dict(time_scale=9.0), dict(pitch_scale=0.1), dict(f0=np.zeros(14)), dict(fs=0.0),
                                dict(time_map=dict(gain=np.ones(5), rate=np.ones(6))), dict(time_map="x"),
                                dict(time_map=dict(gain=np.ones(13), rate=np.zeros(14)))])
def test_noise_fundamental_rejects(kw):
    from eaqhm_amd import noise_fundamental
    args = dict(fs=16000, tau=np.arange(4) * 8.0)
    args.update(kw)
    with pytest.raises(ValueError):
        noise_fundamental(_arrays_model(), args.pop("fs"), args.pop("tau"), **args)


def test_binding_header_and_exports():
    import eaqhm_amd
    from eaqhm_amd import hip
    from conftest import ROOT
    assert hip.ABI_VERSION == 6
    sym = {n: a for n, _, a in hip.SYMBOLS}
    assert len(sym["eaqhm_noise_modulation"]) == 13
    import ctypes as C
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    plain = [P, P, P, I32, I32, I32, P, I32, C.c_uint64, I64, I64, I64, P, I32]      # ctx .. out, accumulate
    assert sym["eaqhm_noise_synth"] == plain + [P, I32, P, P] and len(sym["eaqhm_noise_synth"]) == 18
    with open(os.path.join(ROOT, "include", "eaqhm_hip.h")) as fh:
        header = fh.read()
    assert "int eaqhm_noise_modulation(" in header and "int eaqhm_noise_synth(" in header
    gone = "eaqhm_noise_synth" + "_mod"
    assert gone not in sym and gone not in header
    assert callable(hip.Context.noise_modulation) and callable(hip.Context.noise_synth)
    assert not hasattr(hip.Context, "noise_synth_mod")
    for name in ("eaQHMNoiseModulation", "model_phase", "noise_fundamental"):
        assert callable(getattr(eaqhm_amd, name))


def test_cli_noise_modulation_flag(tmp_path):
    from eaqhm_amd import cli
    a = cli.parser().parse_args(["x.wav", "--noise", "--noise-modulation"])
    assert a.noise and a.noise_modulation == 2
    assert cli.parser().parse_args(["x.wav", "--noise", "--noise-modulation", "4"]).noise_modulation == 4
    assert cli.parser().parse_args(["x.wav", "--noise"]).noise_modulation is None
    missing = str(tmp_path / "missing.wav")
    with pytest.raises(SystemExit):
        cli.main([missing, "--noise-modulation"])                      # needs --noise
    with pytest.raises(SystemExit):
        cli.main([missing, "--noise", "--noise-modulation", "x"])
    with pytest.raises(ValueError):
        cli.main([missing, "--noise", "--noise-modulation", "9"])      # rejected before the analysis
    with pytest.raises(FileNotFoundError):
        cli.main([missing, "--noise", "--noise-modulation", "3"])      # accepted: the analysis starts
