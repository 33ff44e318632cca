"""Pitch-synchronous modulation of the noise on the MI355X (eaQHMNoiseModulation -> eaqhm_noise_modulation,
eaQHMNoiseSynthesis(fundamental=) and eaQHMSynthesis(noise_modulation=True) -> eaqhm_noise_synth with mod) against the NumPy
model of DESIGN.md §10.2 (tests/noise_modulation_ref.py).

Bars: §10's rule for reductions, 100 x the largest deviation between the model run in float64 and in np.longdouble on
the same input, computed when the test runs.  The model sums in the kernel's order, so the kernels differ from it
where cos / sin / sqrt and the division do.  No frame is excluded; the exactly-zero frames must be the same frames.
What the bars came to on the MI355X is recorded by the tests (record_measurement) and tabulated in DESIGN.md §10.2."""
import os

import numpy as np
import pytest
from scipy.io import wavfile

import noise_model_ref as N
import noise_modulation_ref as R
from conftest import GOLDEN, ROOT, load_golden, record_measurement
from test_gpu_model_synthesis import analyse

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


@pytest.fixture(scope="module")
def sa19(amd, tmp_path_factory):
    """(s, s_recon, arrays model) of a fresh SA19 analysis; s is the signal the analysis saw."""
    g = load_golden("sa19_female_default.npz")
    path = os.path.join(GOLDEN, "SA19.WAV")
    fs, x = wavfile.read(path)
    s_recon, _, arrays = analyse(amd, tmp_path_factory.mktemp("m19"), x, fs, "SA19", track=g["swipe_track"])
    fs2, s = amd.read_signal(path)
    assert fs2 == fs == 16000 and len(s) == len(s_recon)
    return s, s_recon, arrays


@pytest.fixture(scope="module")
def synth48k(amd, tmp_path_factory):
    from eaqhm_amd.synth import synth_speech_int16
    x = synth_speech_int16(0.6, 48000)
    s_recon, _, arrays = analyse(amd, tmp_path_factory.mktemp("m48"), x, 48000, "synth48k_0p6s", maxAdpt=1)
    return x / 32768.0, s_recon, arrays


def pulsed_ar():
    """The AR(4) fixture of §10 with a pulsed gain: a one-slot model gliding 180 -> 300 Hz (unvoiced over
    [0.6, 0.7) s), the noise multiplied by g(Theta(n)), g^2 = 1 + 0.8 cos(2 pi Theta - 0.9) + 0.3 cos(4 pi Theta)."""
    det, rec, L = R.glide_model(16000, 2.0, 15)
    e = N.ar_fixture()
    assert len(e) == L
    th = R.phase_at(np.arange(L), R.model_phase(rec, 15, 16000), R.model_f0(rec), 0.0, 15, 16000)
    e = e * np.sqrt(1 + 0.8 * np.cos(2 * np.pi * th - 0.9) + 0.3 * np.cos(4 * np.pi * th))
    t = det["ti"] / 16000.0
    det["amplitudes"][(t >= 0.6) & (t < 0.7)] = 0.0
    return e, det


@pytest.fixture(scope="module")
def residuals(sa19, synth48k):
    """(label, s, s_recon, fs, H, det, M): the three fixtures."""
    e, det = pulsed_ar()
    return [("ar4_pulsed", e, np.zeros(len(e)), 16000, 80, det, 3), ("sa19", sa19[0], sa19[1], 16000, 80, sa19[2], 2),
            ("synth48k", synth48k[0], synth48k[1], 48000, 240, synth48k[2], 8)]


def _model_inputs(amd, det, fs):
    """What the kernel gets per instant, from the host functions: (theta, f0, voiced, step)."""
    m = amd.unpack_model(det)
    K = m["Kmax"]
    return amd.model_phase(det, fs), amd.model_f0(det, fs), (m["records"][:, :K] != 0).any(axis=1), m["step"]


def test_analysis_against_numpy_model(amd, residuals):
    for label, s, s_recon, fs, H, det, M in residuals:
        nz = amd.eaQHMNoiseAnalysis(s, s_recon, fs)
        out = amd.eaQHMNoiseModulation(s, s_recon, nz, det, M)
        Nf = len(nz["sigma"])
        assert out["mod_harmonics"] == M and out["mod"].shape == (Nf, 2 * M) and out["mod"].dtype == np.float64
        for key in ("sigma", "refl"):
            assert np.array_equal(out[key], nz[key])
        assert (out["hop"], out["order"], out["fs"], out["length"]) == (H, nz["order"], float(fs), len(s))
        theta, f0, voiced, step = _model_inputs(amd, det, fs)
        e = np.asarray(s, dtype=np.float64) - s_recon
        ref = R.analyse(e, H, M, theta, f0, voiced, 0.0, step, fs)
        ref_l = R.analyse(e, H, M, theta, f0, voiced, 0.0, step, fs, np.longdouble)
        zero, zero_ref = np.all(out["mod"] == 0, axis=1), np.all(ref == 0, axis=1)
        dev = float(np.abs(ref - ref_l).max())
        err = float(np.abs(out["mod"] - ref).max())
        c1 = np.hypot(ref[:, 0], ref[:, 1])
        print("noise modulation %s: frames %d zero %d M %d mean|c_1| %.4f max|c| %.4f  model dev %.3g gpu err %.3g"
              % (label, Nf, int(zero_ref.sum()), M, float(c1[~zero_ref].mean()), float(np.abs(ref).max()), dev, err))
        record_measurement("noise_modulation_vs_numpy_%s" % label, frames=Nf, zero_frames=int(zero_ref.sum()),
                           harmonics=M, mean_abs_c1=float(c1[~zero_ref].mean()), max_abs_c=float(np.abs(ref).max()),
                           model_dev=dev, gpu_err=err)
        assert np.array_equal(zero, zero_ref), label
        assert np.array_equal(zero_ref, np.all(ref_l == 0, axis=1))
        assert dev > 0 and err <= 100 * dev, (label, err, dev)
        # the coefficients do not depend on how many are asked for
        if M > 1:
            assert np.array_equal(amd.eaQHMNoiseModulation(s, s_recon, nz, det, 1)["mod"], out["mod"][:, :2])
    label, s, s_recon, fs, H, det, M = residuals[0]
    assert int(np.all(amd.eaQHMNoiseModulation(s, s_recon, amd.eaQHMNoiseAnalysis(s, s_recon, fs), det, M)["mod"] == 0,
                      axis=1).sum()) >= 30                      # the silent stretch and the unvoiced one


def _cases(amd, det, fs, H, L):
    """(name, tau, L_out, theta, nu) at rho 1, 0.5, 2 (beta 1, 1.3, 0.8) and a contour pair."""
    from eaqhm_amd.model import contour_time_map, noise_time_map, noise_time_map_contour
    cases = []
    for rho, beta in ((1.0, 1.0), (0.5, 1.3), (2.0, 0.8)):
        Lo = int(np.rint(rho * L))
        tau = noise_time_map(H, Lo, rho)
        cases.append(("rho%g" % rho, tau, Lo) + amd.noise_fundamental(det, fs, tau, time_scale=rho, pitch_scale=beta))
    m = amd.unpack_model(det)
    n, step = len(m["ti"]), m["step"]
    x = np.arange(n) / (n - 1)
    beta_c = 0.8 + 0.5 * x
    tm = contour_time_map(1.1 + 0.5 * np.sin(2 * np.pi * 3 * x), beta_c, step, L)
    tau = noise_time_map_contour(H, tm, step)
    cases.append(("contour", tau, tm["L_out"]) + amd.noise_fundamental(det, fs, tau, time_map=tm, pitch_scale=beta_c))
    return cases


def test_synthesis_against_numpy_model(amd, residuals):
    for label, s, s_recon, fs, H, det, M in (residuals[0], residuals[2]):
        nz = amd.eaQHMNoiseModulation(s, s_recon, amd.eaQHMNoiseAnalysis(s, s_recon, fs), det, M)
        for name, tau, L_out, theta, nu in _cases(amd, det, fs, H, len(s)):
            out = amd.eaQHMNoiseSynthesis(nz, tau, L_out, seed=77, fundamental=(theta, nu))
            plain = amd.eaQHMNoiseSynthesis(nz, tau, L_out, seed=77)
            ref = R.synth_mod(nz["sigma"], nz["refl"], H, tau, L_out, 77, nz["mod"], theta, nu)
            ref_l = R.synth_mod(nz["sigma"], nz["refl"], H, tau, L_out, 77, nz["mod"], theta, nu, np.longdouble)
            top = float(np.abs(ref).max())
            dev = float(np.abs(ref - ref_l).max() / top)
            err = float(np.abs(out - ref).max() / top)
            moved = float(np.abs(out - plain).max() / top)
            print("modulated noise synthesis %s %s: L_out %d model dev %.3g gpu err %.3g (modulation moves %.3g)"
                  % (label, name, L_out, dev, err, moved))
            record_measurement("noise_synth_mod_vs_numpy_%s_%s" % (label, name), model_dev=dev, gpu_err=err, moved=moved)
            assert out.shape == ref.shape == (L_out,) and out.dtype == np.float64 and top > 0 and dev > 0
            assert moved > 1e-3, (label, name)                  # the comparison is of a modulated signal
            assert err <= 100 * dev, (label, name, err, dev)


def test_zero_mod_ranges_and_accumulate_bit_for_bit(amd):
    import torch
    from eaqhm_amd.functions import _ctx
    e, det = pulsed_ar()
    fs = 16000
    nz = amd.eaQHMNoiseModulation(e, np.zeros(len(e)), amd.eaQHMNoiseAnalysis(e, np.zeros(len(e)), fs), det, 3)
    H, p, Nf = nz["hop"], nz["order"], len(nz["sigma"])
    L_out = 40013
    tau = amd.noise_time_map(H, L_out, 1.25)
    fund = amd.noise_fundamental(det, fs, tau, time_scale=1.25, pitch_scale=0.9)
    plain = amd.eaQHMNoiseSynthesis(nz, tau, L_out, seed=5)
    assert np.array_equal(amd.eaQHMNoiseSynthesis({k: v for k, v in nz.items() if not k.startswith("mod")}, tau, L_out,
                                                  seed=5), plain)          # without fundamental the keys change nothing
    zero = dict(nz, mod=np.zeros_like(nz["mod"]))
    assert np.array_equal(amd.eaQHMNoiseSynthesis(zero, tau, L_out, seed=5, fundamental=fund), plain)
    a = amd.eaQHMNoiseSynthesis(nz, tau, L_out, seed=5, fundamental=fund)
    assert not np.array_equal(a, plain) and np.array_equal(a, amd.eaQHMNoiseSynthesis(nz, tau, L_out, 5, fund))
    for cuts in ((0, 13337, 29999, L_out), (0, 80 * 100, 80 * 300 - 1, L_out), (0, 1, L_out - 1, L_out)):
        parts = amd.eaQHMNoiseSynthesis(nz, tau, L_out, seed=5, fundamental=fund, _ranges=list(zip(cuts[:-1], cuts[1:])))
        assert np.array_equal(parts, a), cuts
    c = _ctx(0)
    base = np.random.default_rng(3).normal(size=L_out)
    buf = torch.as_tensor(base.copy(), device=c.device)
    dv = [torch.as_tensor(np.ascontiguousarray(x), device=c.device)
          for x in (nz["sigma"], nz["refl"], tau, nz["mod"], fund[0], fund[1])]
    for t_lo, t_hi in ((0, 20000), (20000, L_out)):
        c.noise_synth(dv[0], dv[1], Nf, H, p, dv[2], len(tau), 5, L_out, t_lo, t_hi, buf, accumulate=True,
                      mod=(dv[3], 3, dv[4], dv[5]))
    assert np.array_equal(buf.cpu().numpy(), base + a)
    # the floor: coefficients that drive g^2 negative, against the model (cos, sin and sqrt apart: 1e-12 of the maximum)
    deep = dict(nz, mod=np.tile([0.9, 0.0, 0.0, 0.0, 0.0, 0.0], (Nf, 1)))
    out = amd.eaQHMNoiseSynthesis(deep, tau, L_out, seed=5, fundamental=fund)
    ref = R.synth_mod(nz["sigma"], nz["refl"], H, tau, L_out, 5, deep["mod"], fund[0], fund[1])
    assert np.all(np.isfinite(out)) and np.abs(out - ref).max() <= 1e-12 * np.abs(ref).max()


def test_synthesis_with_modulated_noise_is_the_sum_of_the_two_calls(amd, sa19):
    from eaqhm_amd.model import contour_time_map, noise_time_map, noise_time_map_contour
    s, s_recon, det = sa19
    fs, L = 16000, len(s)
    plain = amd.eaQHMNoiseAnalysis(s, s_recon, fs)
    nz = amd.eaQHMNoiseModulation(s, s_recon, plain, det)
    assert nz["mod_harmonics"] == 2
    H = nz["hop"]
    n = len(det["ti"])
    step = int(det["ti"][1] - det["ti"][0])
    f0_user = amd.model_f0(det, fs) * 1.01
    for kw in (dict(), dict(time_scale=1.5), dict(time_scale=0.6, pitch_scale=1.2, formant_scale=0.9),
               dict(time_scale=1.5, pitch_scale=0.8, phase="shape"),
               dict(time_scale=1.2, pitch_scale=1.25, phase="shape", f0=f0_user)):
        rho, beta = kw.get("time_scale", 1.0), kw.get("pitch_scale", 1.0)
        L_out = int(np.rint(rho * L))
        tau = noise_time_map(H, L_out, rho)
        fund = amd.noise_fundamental(det, fs, tau, time_scale=rho, pitch_scale=beta, f0=kw.get("f0"))
        both = amd.eaQHMSynthesis(det, fs, L, noise=nz, noise_seed=9, noise_modulation=True, **kw)
        only = amd.eaQHMSynthesis(det, fs, L, **kw)
        noise = amd.eaQHMNoiseSynthesis(nz, tau, L_out, 9, fund)
        assert np.array_equal(both, only + noise), kw
        # noise_modulation=False with the mod-carrying dict is the call with the plain dict
        off = amd.eaQHMSynthesis(det, fs, L, noise=nz, noise_seed=9, noise_modulation=False, **kw)
        assert np.array_equal(off, amd.eaQHMSynthesis(det, fs, L, noise=plain, noise_seed=9, **kw)), kw
        assert not np.array_equal(off, both)
    x = np.arange(n) / (n - 1)
    rho_c, beta_c = 1.1 + 0.5 * np.sin(2 * np.pi * 3 * x), 0.8 + 0.5 * x
    tm = contour_time_map(rho_c, beta_c, step, L)
    tau = noise_time_map_contour(H, tm, step)
    fund = amd.noise_fundamental(det, fs, tau, time_map=tm, pitch_scale=beta_c)
    noise = amd.eaQHMNoiseSynthesis(nz, tau, tm["L_out"], 9, fund)
    cut = tm["L_out"] // 3
    for kw in (dict(), dict(phase="shape")):
        both = amd.eaQHMSynthesis(det, fs, L, time_scale=rho_c, pitch_scale=beta_c, noise=nz, noise_seed=9,
                                  noise_modulation=True, **kw)
        only = amd.eaQHMSynthesis(det, fs, L, time_scale=rho_c, pitch_scale=beta_c, **kw)
        assert np.array_equal(both, only + noise), kw
        parts = amd.eaQHMSynthesis(det, fs, L, time_scale=rho_c, pitch_scale=beta_c, noise=nz, noise_seed=9,
                                   noise_modulation=True, _ranges=[(0, cut), (cut, 2 * cut), (2 * cut, tm["L_out"])], **kw)
        assert np.array_equal(parts, both), kw
    # noise_formant=True: the warp carries mod through, and the sum holds with the warped model
    kw = dict(time_scale=1.3, pitch_scale=1.1, formant_scale=0.85)
    warped = amd.eaQHMNoiseWarp(nz, amd.noise_formant_contour(nz, det, 0.85))
    assert np.array_equal(warped["mod"], nz["mod"]) and warped["mod_harmonics"] == 2
    assert not np.array_equal(warped["refl"], nz["refl"])
    L_out = int(np.rint(1.3 * L))
    tau = noise_time_map(H, L_out, 1.3)
    fund = amd.noise_fundamental(det, fs, tau, time_scale=1.3, pitch_scale=1.1)
    both = amd.eaQHMSynthesis(det, fs, L, noise=nz, noise_seed=9, noise_formant=True, noise_modulation=True, **kw)
    assert np.array_equal(both, amd.eaQHMSynthesis(det, fs, L, **kw) + amd.eaQHMNoiseSynthesis(warped, tau, L_out, 9, fund))


def test_sa19_modulated_noise_keeps_the_residuals_power(amd, sa19):
    """§10's check with the modulation on: per 100 ms block where the residual's power is above 1e-3 of its largest
    block's, the synthesised noise's power is within +-4 dB of the residual's.  The modulation must not move the power:
    the mean of g^2 over a period is 1."""
    from eaqhm_amd.model import noise_time_map
    s, s_recon, det = sa19
    fs, L = 16000, len(s)
    e = s - s_recon
    nz = amd.eaQHMNoiseModulation(s, s_recon, amd.eaQHMNoiseAnalysis(s, s_recon, fs), det)
    tau = noise_time_map(nz["hop"], L, 1.0)
    y = amd.eaQHMNoiseSynthesis(nz, tau, L, seed=1, fundamental=amd.noise_fundamental(det, fs, tau))
    y0 = amd.eaQHMNoiseSynthesis(nz, tau, L, seed=1)
    blk = fs // 10
    nb = L // blk
    pe = np.array([np.mean(e[i * blk:(i + 1) * blk] ** 2) for i in range(nb)])
    py = np.array([np.mean(y[i * blk:(i + 1) * blk] ** 2) for i in range(nb)])
    p0 = np.array([np.mean(y0[i * blk:(i + 1) * blk] ** 2) for i in range(nb)])
    good = pe > 1e-3 * pe.max()
    ratio = 10 * np.log10(py[good] / pe[good])
    shift = 10 * np.log10(py[good] / p0[good])
    c1 = np.hypot(nz["mod"][:, 0], nz["mod"][:, 1])
    print("SA19 modulated noise power: %d of %d blocks, ratio %.2f .. %.2f dB; against the unmodulated noise "
          "%.2f .. %.2f dB; mean |c_1| %.3f" % (int(good.sum()), nb, ratio.min(), ratio.max(), shift.min(), shift.max(),
                                                float(c1[c1 > 0].mean())))
    record_measurement("noise_modulation_sa19_block_power", blocks=int(good.sum()), ratio_min_db=float(ratio.min()),
                       ratio_max_db=float(ratio.max()), shift_min_db=float(shift.min()), shift_max_db=float(shift.max()),
                       mean_abs_c1=float(c1[c1 > 0].mean()))
    assert good.sum() >= 5
    assert ratio.min() >= -4.0 and ratio.max() <= 4.0, (ratio.min(), ratio.max())


def test_entry_points_reject_bad_arguments(amd):
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)

    def z(*shape, dtype=torch.float64):
        return torch.zeros(shape, dtype=dtype, device=c.device)

    L, H, p, n = 1000, 8, 4, 67
    Nf = (L - 1) // H + 1
    e, sigma, refl, tau, out, mod, th, f0 = z(L), z(Nf), z(Nf, p), z(Nf), z(L), z(Nf, 16), z(n), z(n)
    vo = z(n, dtype=torch.uint8)
    c.noise_modulation(e, L, H, th, f0, vo, n, 0.0, 15.0, 16000.0, 8, mod)          # the good calls
    c.noise_synth(sigma, refl, Nf, H, p, tau, Nf, 0, L, 0, L, out, mod=(mod, 8, tau, tau))
    c.sync()
    for M in (0, 9, -1):
        with pytest.raises(RuntimeError, match="error -1"):
            c.noise_modulation(e, L, H, th, f0, vo, n, 0.0, 15.0, 16000.0, M, mod)
        with pytest.raises(RuntimeError, match="error -1"):
            c.noise_synth(sigma, refl, Nf, H, p, tau, Nf, 0, L, 0, L, out, mod=(mod, M, tau, tau))
    for kw in (dict(hop=0), dict(hop=1025), dict(L=0), dict(n=0), dict(step=0.0), dict(fs=0.0)):
        a = dict(L=L, hop=H, n=n, step=15.0, fs=16000.0)
        a.update(kw)
        with pytest.raises(RuntimeError, match="error -1"):
            c.noise_modulation(e, a["L"], a["hop"], th, f0, vo, a["n"], 0.0, a["step"], a["fs"], 2, mod)
    with pytest.raises(RuntimeError, match="error -1"):
        c.noise_modulation(e, L, H, None, f0, vo, n, 0.0, 15.0, 16000.0, 2, mod)
    for bad in ((None, tau, tau), (mod, None, tau), (mod, tau, None)):
        with pytest.raises(RuntimeError, match="error -1"):
            c.noise_synth(sigma, refl, Nf, H, p, tau, Nf, 0, L, 0, L, out, mod=(bad[0], 2, bad[1], bad[2]))
    for Nq, t_lo, t_hi in ((Nf - 1, 0, L), (Nf, -1, L), (Nf, 0, L + 1), (Nf, 5, 5)):
        with pytest.raises(RuntimeError, match="error -1"):
            c.noise_synth(sigma, refl, Nf, H, p, tau, Nq, 0, L, t_lo, t_hi, out, mod=(mod, 2, tau, tau))
    assert c.abi_version == 6


def test_optional_groups_given_in_part_are_rejected(amd):
    """A partial mod group of eaqhm_noise_synth, a partial curve group and a partial shape group of eaqhm_modify_synth:
    EAQHM_EINVAL from the argument checks, which return before any launch, and `out` as it was."""
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)

    def z(*shape, dtype=torch.float64):
        return torch.zeros(shape, dtype=dtype, device=c.device)

    def rejected(call):
        out = torch.full((L,), 7.0, dtype=torch.float64, device=c.device)
        with pytest.raises(RuntimeError, match="error -1: eaqhm_(noise|modify)_synth: bad argument"):
            call(out)
        c.sync()
        assert bool((out == 7.0).all())

    L, H, p, n, K, D = 1000, 8, 4, 67, 3, 15
    Nf = (L - 1) // H + 1
    sigma, refl, tau, mod = z(Nf), z(Nf, p), z(Nf), z(Nf, 4)
    for m, th, nu in ((None, tau, tau), (mod, None, tau), (mod, tau, None), (mod, None, None), (None, None, tau)):
        rejected(lambda out: c.noise_synth(sigma, refl, Nf, H, p, tau, Nf, 0, L, 0, L, out, mod=(m, 2, th, nu)))
    rec, code, mom = z(n, 3 * K + 1), z(n * K, dtype=torch.uint8), z(n * (K + 1))
    amp, R, ph0, v = z(n * K), z(n * K), z(n * K), z(n)
    for C_, rate, gain in ((None, v, v), (v, None, v), (v, v, None), (v, None, None), (None, None, v)):
        rejected(lambda out: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, 16000.0, 1.0, 1.0, L, 0, L, out,
                                            curve=(C_, rate, gain, 1.0)))
    for f0, S in ((v, None), (None, v)):
        rejected(lambda out: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, 16000.0, 1.0, 1.0, L, 0, L, out,
                                            shape=(f0, S)))
        rejected(lambda out: c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, 16000.0, 1.0, 1.0, L, 0, L, out,
                                            curve=(v, v, v, 1.0), shape=(f0, S)))


def test_cli_noise_modulation_writes_resynthesis(amd, tmp_path):
    import shutil
    from eaqhm_amd import cli
    wav = str(tmp_path / "SA19.WAV")
    shutil.copy(os.path.join(GOLDEN, "SA19.WAV"), wav)
    assert cli.main([wav, "--gender", "female", "--max-adpt", "1", "--noise", "--noise-seed", "3"]) == 0
    _, plain = wavfile.read(str(tmp_path / "SA19_resynthesis.wav"))
    assert cli.main([wav, "--gender", "female", "--max-adpt", "1", "--noise", "--noise-seed", "3",
                     "--noise-modulation"]) == 0
    fs, y = wavfile.read(str(tmp_path / "SA19_resynthesis.wav"))
    assert fs == 16000 and y.dtype == np.float32 and y.shape == plain.shape and np.all(np.isfinite(y))
    assert not np.array_equal(y, plain)
    assert 0.5 < np.std(y) / np.std(plain) < 2.0


def test_record_probe_numbers(amd, synth48k):
    """Device times of the modulation analysis and the modulated synthesis beside the plain ones on the 0.6 s model at
    48 kHz (evidence, not assertions; the 60 s numbers come from tools/model_synthesis_probe.py --noise-modulation)."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from model_synthesis_probe import noise_modulation_rows, prepare
    s, s_recon, arrays = synth48k
    st = prepare(torch, arrays, 48000, len(s), reps=3)
    rows = noise_modulation_rows(torch, st, s - s_recon, reps=3)
    assert rows[0]["modulation_ms"] > 0 and rows[0]["analyse_ms"] > 0 and rows[0]["hop"] == 240
    for row in rows:
        record_measurement("noise_modulation_probe_synth48k_0p6s_%s" % row["setting"],
                           **{k: v for k, v in row.items() if k != "setting"})
    assert all(r["noise_synth_mod_ms"] > 0 and r["noise_synth_ms"] > 0 for r in rows[1:])
