"""The discrete cepstrum on an all-pass warped axis on the MI355X: the *_warped entry points behind
cep_warp= of model_cepstrum, cepstrum_envelope, cepstrum_phase, eaQHMSynthesis(envelope=), model_from_parameters,
model_parameters and noise_from_cepstrum, against the NumPy model (tests/cepstrum_warp_ref.py, which takes the warp in
its atan2 form; the kernels take it through the rational map).  Hand-built models only: no analysis runs.

Bars.  Fit: §10's rule, per case at most 100 x the largest coefficient difference between the model's fit in float64
and in np.longdouble on the same input, computed when the test runs; the normal equations, taken in np.longdouble, are
held to the same bar; no instant is left out.  Readouts (C, Phi, ln |a| of a built model): per row the larger of §9.5's
1e-12 x (|c_0| + 2 sum |c_p|) and 100 x the model's float64-to-longdouble difference in that case (the warp's slope, up
to (1 + |a|) / (1 - |a|) = 19, carries the rounding of the frequency into the angle).  Built phases: 100 x the model's
difference.  Synthesis: 1e-8 of the peak, the bar of test_gpu_model_cepstrum.  Noise: test_gpu_noise_cepstrum's 100 x
rule against the warped model; against the linear route that rule plus the tail the move to the warped axis cuts off."""
import numpy as np
import pytest

import cepstrum_warp_ref as W
import model_cepstrum_ref as CR
import model_formant_ref as MF
import model_shape_ref as MS
import model_synthesis_ref as M
import noise_cepstrum_ref as NR
from conftest import record_measurement

pytestmark = pytest.mark.gpu

LD = np.longdouble
HAND_X = np.array([1000.0, 3000.0, 6000.0])      # the hand map of test_gpu_formant_warp
HAND_Y = np.array([1200.0, 3500.0, 6400.0])
LAMS = (5e-4, 1e-6)
SMALL_WARPS = (0.42, -0.3, 0.9)
WIDE_WARPS = (0.5946, 0.77)


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


# ---- the models of test_gpu_model_cepstrum, rebuilt here
def _det(ti, am, fm, ph, a0):
    return dict(ti=ti, isVoiced=np.ones(len(ti), bool), a0=a0, amplitudes=am, frange=fm, pk=ph)


def small_model():
    """9 instants (not a multiple of the 4 waves of a block), Kmax 5, step 80 at 16 kHz.  Slots at 400, 2800, 3000,
    3000 (tied in frequency) and 7000 Hz; instant 4 has no active partial, instant 8 a single node (slot 1), slot 0 is
    missing at instant 6."""
    n, D, fs = 9, 80, 16000
    ti = np.arange(n) * D
    f = np.array([400.0, 2800.0, 3000.0, 3000.0, 7000.0])
    am = np.exp(np.array([-3.0, -4.5, -3.5, -5.0, -6.0])[None, :] + 0.05 * np.arange(n)[:, None])
    fm = np.tile(f, (n, 1))
    ph = np.angle(np.exp(1j * 2 * np.pi * f[None, :] * ti[:, None] / fs)) + 0.3 * np.arange(5)[None, :]
    am[4] = 0.0
    am[8, [0, 2, 3, 4]] = 0.0
    am[6, 0] = 0.0
    return _det(ti, am, fm, ph, 0.001 * np.arange(n)), fs, (n - 1) * D + 1


def harmonic_model(n, K, f0, fs, step=80, jitter=0.0):
    """n instants of K harmonics of f0 with a formant-shaped ln am that moves a little from instant to instant."""
    ti = np.arange(n) * step
    k = np.arange(1, K + 1)
    fm = f0 * k[None, :] * (1.0 + jitter * np.sin(0.7 * np.arange(n))[:, None])
    lna = (-3.0 - fm / 5000.0 + 2.0 * np.exp(-((fm - (700.0 + 20.0 * np.arange(n)[:, None])) / 300.0) ** 2)
           + 1.5 * np.exp(-((fm - 2400.0) / 500.0) ** 2) + 0.2 * np.sin(1.3 * k[None, :] + np.arange(n)[:, None]))
    ph = np.angle(np.exp(1j * 2 * np.pi * fm * ti[:, None] / fs))
    return _det(ti, np.exp(lna), fm, ph, np.zeros(n)), fs, (n - 1) * step + 1


def wide_model():
    """6 instants, Kmax 148 at 48 kHz: three lane chunks of nodes, harmonics of 160 Hz."""
    return harmonic_model(6, 148, 160.0, 48000)


def other_model():
    """The source of the supplied envelopes: 9 instants, Kmax 12, harmonics of 310 Hz; instant 7 has no active partial,
    so its row is the empty envelope."""
    det, fs, L = harmonic_model(9, 12, 310.0, 16000, jitter=0.01)
    det["amplitudes"][7] = 0.0
    return det, fs, L


MODELS = {"small": small_model, "wide": wide_model, "other": other_model}


def _records(det):
    from eaqhm_amd.model import unpack_model
    m = unpack_model(det)
    return m["records"], m["Kmax"], m["step"]


_REF = {}


def reference_fit(name, P, lam, a):
    """(float64 fit, np.longdouble fit, their largest coefficient difference) of a model on the axis a: computed once
    per case and shared."""
    key = (name, P, lam, a)
    if key not in _REF:
        det, fs, _ = MODELS[name]()
        rec = _records(det)[0]
        c64, cld = W.fit(rec, fs, P, lam, a), W.fit(rec, fs, P, lam, a, LD)
        fin = np.isfinite(c64)
        assert np.array_equal(fin, np.isfinite(cld))
        _REF[key] = (c64, cld, float(np.abs(c64[fin] - cld[fin]).max()))
    return _REF[key]


# ---- the fit
def _check_fit(amd, name, P, lam, a):
    det, fs, _ = MODELS[name]()
    rec, K, _ = _records(det)
    got = amd.model_cepstrum(det, fs, P, lam, cep_warp=a)
    c64, cld, dev = reference_fit(name, P, lam, a)
    assert got.shape == c64.shape == (len(rec), P + 1) and got.dtype == np.float64
    empty = ~((rec[:, :K] != 0) & (rec[:, K:2 * K] > 0)).any(axis=1)
    assert np.all(np.isneginf(got[empty, 0])) and np.all(got[empty, 1:] == 0)          # exactly (-inf, 0, .., 0)
    assert np.all(np.isfinite(got[~empty]))
    err = float(np.abs(got[~empty] - c64[~empty]).max())                                # every non-empty instant
    worst = 0.0
    for i in np.flatnonzero(~empty):
        G, b = W.system(*W.nodes(rec[i, :K], rec[i, K:2 * K], fs, a, LD), P, lam, LD)
        worst = max(worst, float(np.abs(G @ got[i].astype(LD) - b).max() / np.abs(G).sum(axis=1).max()))
    print("warped fit %s a %g P %d lam %g: model dev %.3g gpu err %.3g (bar %.3g) normal equations %.3g"
          % (name, a, P, lam, dev, err, 100 * dev, worst))
    record_measurement("cepwarp_fit_vs_numpy_%s_a%g_P%d_lam%g" % (name, a, P, lam), model_dev=dev, gpu_err=err,
                       bar=100 * dev, normal_equations=worst)
    assert dev > 0
    assert err <= 100 * dev, (name, a, P, lam, err, dev)
    assert worst <= 100 * dev, (name, a, P, lam, worst, dev)
    return got


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("P", [1, 5, 63])
@pytest.mark.parametrize("a", SMALL_WARPS)
def test_fit_small(amd, a, P, lam):
    """P = 5 and 63: more coefficients than the instants have nodes (5 at most, 1 at instant 8)."""
    got = _check_fit(amd, "small", P, lam, a)
    assert np.isneginf(got[4, 0]) and np.all(np.isfinite(got[[8, 6]]))
    det, fs, _ = small_model()
    assert not np.array_equal(got, amd.model_cepstrum(det, fs, P, lam))                # another axis, other rows


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("P", [24, 63])
@pytest.mark.parametrize("a", WIDE_WARPS)
def test_fit_wide(amd, a, P, lam):
    _check_fit(amd, "wide", P, lam, a)


# ---- cep_warp = 0.0 is the call without it
def test_zero_warp_returns_the_bits_of_the_plain_call(amd):
    det, fs, L = small_model()
    odet, ofs, _ = other_model()
    C = amd.model_cepstrum(odet, ofs, 18)
    grid = np.linspace(0.0, 0.6 * fs, 33)
    assert np.array_equal(amd.model_cepstrum(odet, ofs, 18, cep_warp=0.0), C)
    assert np.array_equal(amd.cepstrum_envelope(C, fs, grid, 1.2, cep_warp=0.0), amd.cepstrum_envelope(C, fs, grid, 1.2))
    assert np.array_equal(amd.cepstrum_phase(C, fs, grid, formant_warp=(HAND_X, HAND_Y), cep_warp=0.0),
                          amd.cepstrum_phase(C, fs, grid, formant_warp=(HAND_X, HAND_Y)))
    kw = dict(time_scale=1.5, pitch_scale=1.2, phase="shape", envelope=C)
    assert np.array_equal(amd.eaQHMSynthesis(det, fs, L, cep_warp=0.0, **kw), amd.eaQHMSynthesis(det, fs, L, **kw))
    p, q = amd.model_parameters(odet, ofs, 18), amd.model_parameters(odet, ofs, 18, cep_warp=0.0)
    assert sorted(p) == sorted(q) and all(np.array_equal(p[k], q[k]) for k in p)
    b0 = amd.model_from_parameters(p["f0"], p["ceps"], p["fs"], p["step"], voiced=p["voiced"])
    b1 = amd.model_from_parameters(p["f0"], p["ceps"], p["fs"], p["step"], voiced=p["voiced"], cep_warp=0.0)
    assert all(np.array_equal(b0[k], b1[k]) for k in b0)
    sigma, refl, _ = NR.pole_frames(9, 18, 0.7, seed=1, silent=(0, 4, 8))
    rows = amd.noise_cepstrum(NR.noise_model(sigma, refl), 63)
    n0, n1 = amd.noise_from_cepstrum(rows, 80, 16000), amd.noise_from_cepstrum(rows, 80, 16000, cep_warp=0.0)
    assert np.array_equal(n0["sigma"], n1["sigma"]) and np.array_equal(n0["refl"], n1["refl"])


# ---- the readouts
def _scale_of(C):
    c0 = np.where(np.isfinite(C[:, 0]), C[:, 0], 0.0)
    return np.abs(c0) + 2 * np.abs(C[:, 1:]).sum(axis=1)


def _row_bar(C, ref64, refld):
    """Per row: the larger of the existing readout bar and 100 x the model's own float64-to-longdouble difference."""
    with np.errstate(invalid="ignore"):
        dev = np.abs(ref64.astype(LD) - refld).astype(np.float64)
    dev = np.where(np.isfinite(dev), dev, 0.0).max(axis=1)
    return np.maximum(1e-12 * _scale_of(C), 100 * dev), dev


def _check_readouts(amd, label, C, fs, a, grid):
    n = len(C)
    empty = np.isneginf(C[:, 0])
    cases = [("plain", {}, {}), ("alpha0.85", dict(formant_scale=0.85), dict(alpha=0.85)),
             ("alpha1.2", dict(formant_scale=1.2), dict(alpha=1.2)),
             ("hand_map", dict(formant_warp=(HAND_X, HAND_Y)), dict(warp=(HAND_X, HAND_Y)))]
    out = {}
    for case, kw, rkw in cases:
        for what, fn, ref in (("envelope", amd.cepstrum_envelope, W.envelope), ("phase", amd.cepstrum_phase, W.envelope_phase)):
            got = fn(C, fs, grid, cep_warp=a, **kw)
            r64, rld = ref(C, fs, grid, a, **rkw), ref(C, fs, grid, a, dtype=LD, **rkw)
            assert got.shape == r64.shape == (n, len(grid)) and got.dtype == np.float64
            if what == "envelope":
                assert np.all(np.isneginf(got[empty])) and np.all(np.isfinite(got[~empty]))
            else:
                assert np.all(got[empty] == 0) and np.all(got[:, 0] == 0)                 # the empty row; Phi(0) = 0
            bar, dev = _row_bar(C, r64, rld)
            rel = (np.abs(got[~empty] - r64[~empty]).max(axis=1) / bar[~empty]).max()
            print("warped %s %s a %g %s: worst error / bar %.3g (model dev %.3g)" % (what, label, a, case, rel, dev.max()))
            record_measurement("cepwarp_%s_vs_numpy_%s_a%g_%s" % (what, label, a, case), worst_error_over_bar=float(rel),
                               model_dev=float(dev.max()))
            assert rel <= 1.0, (what, label, a, case, rel)
            out[what, case] = got
    return out


@pytest.mark.parametrize("a", SMALL_WARPS)
def test_readouts_against_numpy(amd, a):
    """33 points from 0 to 0.6 fs: the hold past fs/2 is on the grid.  The rows are the model's fit of other_model on
    the axis a (row 7 is the empty row)."""
    _, fs, _ = other_model()
    C = reference_fit("other", 18, 5e-4, a)[0]
    assert np.isneginf(C[7, 0])
    grid = np.linspace(0.0, 0.6 * fs, 33)
    got = _check_readouts(amd, "other_P18", C, fs, a, grid)
    past = grid >= fs / 2
    for what, fn in (("envelope", amd.cepstrum_envelope), ("phase", amd.cepstrum_phase)):
        at = fn(C, fs, [fs / 2.0], cep_warp=a)
        assert past.sum() > 1 and np.array_equal(got[what, "plain"][:, past], np.repeat(at, past.sum(), axis=1))     # held
        assert not np.array_equal(got[what, "plain"], fn(C, fs, grid))                 # the axis matters
    assert np.abs(got["phase", "plain"]).max() > 0.1


@pytest.mark.parametrize("a", WIDE_WARPS)
def test_readouts_at_the_highest_order(amd, a):
    _, fs, _ = wide_model()
    C = reference_fit("wide", 63, 5e-4, a)[0]
    _check_readouts(amd, "wide_P63", C, fs, a, np.linspace(0.0, 0.6 * fs, 33))


def test_the_hold_below_zero(amd):
    """The public functions take no frequency below 0; the entry points hold one at 0, on the warped axis as well."""
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    _, fs, _ = other_model()
    C = reference_fit("other", 18, 5e-4, 0.42)[0]
    grid = np.array([-0.1 * fs, -1.0, 0.0, 100.0])
    C_d, f_d = torch.as_tensor(C, device=c.device), torch.as_tensor(grid, device=c.device)
    for fn in (c.cepstrum_envelope_warped, c.cepstrum_phase_warped):
        out = torch.empty((len(C), 4), dtype=torch.float64, device=c.device)
        fn(C_d, len(C), 18, float(fs), f_d, 4, out, 0.42)
        got = out.cpu().numpy()
        assert np.array_equal(got[:, 0], got[:, 2]) and np.array_equal(got[:, 1], got[:, 2])
        assert not np.array_equal(got[:, 3], got[:, 2])


# ---- amplitudes and synthesis with a supplied warped envelope
@pytest.mark.parametrize("a", SMALL_WARPS)
def test_synthesis_with_a_supplied_warped_envelope(amd, a):
    det, fs, L = small_model()
    rec, K, D = _records(det)
    C = reference_fit("other", 18, 5e-4, a)[0]
    for label, rho, beta, kw in (("unit", 1.0, 1.0, {}), ("scaled_shape", 1.5, 1.2, dict(phase="shape"))):
        out = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, envelope=C, cep_warp=a, **kw)
        Ap = W.amplitudes(rec[:, :K], rec[:, K:2 * K], fs, beta, C, a)
        with MF._amplitudes(Ap):
            ref = MS.synthesize_shape(rec, D, fs, L, rho, beta) if kw else M.synthesize(rec, D, fs, L, rho, beta, True)
        assert out.shape == ref.shape == (int(np.rint(rho * L)),) and out.dtype == np.float64
        rel = float(np.abs(out - ref).max() / np.abs(ref).max())
        print("warped synthesis a %g %s: max rel %.3g" % (a, label, rel))
        record_measurement("cepwarp_synthesis_vs_numpy_a%g_%s" % (a, label), max_rel=rel)
        assert rel <= 1e-8, (a, label, rel)
        assert not np.array_equal(out, amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, envelope=C, **kw))


def test_amplitudes_under_a_formant_scale_and_map(amd):
    """The formant controls act in Hz before the warp: Context.modify_amp_cepstrum_warped against the model."""
    import torch
    from eaqhm_amd.functions import _ctx
    det, fs, _ = small_model()
    rec_h, K, D = _records(det)
    n, a = len(rec_h), 0.42
    C = reference_fit("other", 18, 5e-4, a)[0]
    am, fm = rec_h[:, :K], rec_h[:, K:2 * K]
    c = _ctx(0)

    def t(x):
        return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=c.device)

    rows = np.tile(HAND_Y, (n, 1))
    bar = 1e-12 * (1.0 + _scale_of(C))
    for label, beta, alpha, warp in (("beta1.25_alpha1.2", 1.25, 1.2, None), ("beta1.25_hand", 1.25, None, (HAND_X, rows))):
        amp = torch.full((n, K), -1.0, dtype=torch.float64, device=c.device)
        c.modify_amp_cepstrum_warped(t(rec_h), n, K, float(fs), t(np.full(n, beta)), t(C), 18, amp, a,
                                     alpha=None if alpha is None else t(np.full(n, alpha)),
                                     warp=None if warp is None else (t(warp[0]), t(warp[1]), 3))
        got = amp.cpu().numpy()
        ref = W.amplitudes(am, fm, fs, beta, C, a, alpha, warp)
        zero = ~((am != 0) & (fm > 0)) | (beta * fm >= fs / 2) | np.isneginf(C[:, :1])
        assert np.array_equal(ref == 0, zero) and np.array_equal(got == 0, zero), label
        rel = np.abs(got / np.where(zero, 1.0, ref) - 1.0)
        rel[zero] = 0.0
        worst = float((rel.max(axis=1) / bar).max())
        record_measurement("cepwarp_amplitudes_vs_numpy_%s" % label, worst_error_over_bar=worst)
        assert worst <= 1.0, (label, worst)


# ---- the model from parameters
def _rows(n, P, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate((-4.0 + 0.3 * rng.standard_normal((n, 1)),
                           rng.standard_normal((n, P)) / (1.0 + np.arange(1, P + 1)) ** 1.2), axis=1)


def build_small(P):
    """test_gpu_model_build's: 9 instants at 16 kHz, step 80: 1, 63, 64, 65, -, 25, 39, -, 82 harmonics; instant 4 is
    unvoiced, instant 7 an empty row."""
    f0 = np.array([5000.0, 125.0, 124.0, 123.0, 150.0, 310.0, 200.0, 180.0, 97.5])
    voiced = np.ones(9, bool)
    voiced[4] = False
    C = _rows(9, P, 11 + P)
    C[7] = 0.0
    C[7, 0] = -np.inf
    return dict(f0=f0, voiced=voiced, ceps=C, fs=16000, step=80, theta0=0.3, a0=0.001 * np.arange(9) * voiced)


def build_wide(P):
    """6 instants at 48 kHz, step 240: 141 to 149 harmonics (160 Hz), three lane chunks."""
    f0 = np.array([170.0, 165.0, 162.0, 161.0, 160.0, 160.0])
    return dict(f0=f0, voiced=np.ones(6, bool), ceps=_rows(6, P, 5 + P), fs=48000, step=240, theta0=0.0, a0=None)


def _mod(d):
    return np.abs(np.angle(np.exp(1j * d)))


@pytest.mark.parametrize("name,P,a", [("small", 18, 0.42), ("small", 18, -0.3), ("small", 63, 0.9),
                                      ("wide", 63, 0.5946), ("wide", 24, 0.77)])
def test_built_records(amd, name, P, a):
    p = (build_small if name == "small" else build_wide)(P)
    n = len(p["f0"])
    for phase in ("minimum", "zero"):
        kw = dict(theta0=p["theta0"], a0=p["a0"], zero_phase=phase == "zero")
        b64 = W.build(p["f0"], p["voiced"], p["ceps"], p["fs"], p["step"], a, **kw)
        bld = W.build(p["f0"], p["voiced"], p["ceps"], p["fs"], p["step"], a, dtype=LD, **kw)
        assert np.array_equal(b64["active"], bld["active"])
        act, K, rec = b64["active"], b64["Kmax"], b64["records"]
        d = (bld["phase"] - b64["phase"].astype(LD)).astype(np.float64)
        dev_ph = float(_mod(d)[act].max())
        det = amd.model_from_parameters(p["f0"], p["ceps"], p["fs"], p["step"], voiced=p["voiced"], phase=phase,
                                        theta0=p["theta0"], a0=p["a0"], cep_warp=a)
        am, fm, pk = det["amplitudes"], det["frange"], det["pk"]
        assert am.shape == fm.shape == pk.shape == (n, K)
        assert np.array_equal(am != 0, act)                                        # the active set, exactly
        assert np.array_equal(fm, rec[:, K:2 * K]) and np.array_equal(det["a0"], rec[:, 3 * K])
        assert np.all(pk[~act] == 0) and np.all(np.abs(pk) <= np.pi)
        lnam64 = np.where(act, b64["lnam"].astype(np.float64), 0.0)
        lnamld = np.where(act, bld["lnam"], LD(0))
        bar, dev_ln = _row_bar(p["ceps"], lnam64, lnamld)
        bar = np.broadcast_to(bar[:, None], (n, K))
        e_ln = float((np.abs(np.log(am[act]) - lnam64[act]) / bar[act]).max())     # every active cell
        e_ph = float(_mod(pk - rec[:, 2 * K:3 * K])[act].max())
        label = "%s_P%d_a%g_%s" % (name, P, a, phase)
        print("warped build %s: ln am error / bar %.3g; model dev %.3g, phase error %.3g" % (label, e_ln, dev_ph, e_ph))
        record_measurement("cepwarp_build_vs_numpy_%s" % label, ln_am_error_over_bar=e_ln, model_dev=dev_ph,
                           phase_error=e_ph, ln_am_model_dev=float(dev_ln.max()))
        assert dev_ph > 0
        assert e_ln <= 1.0, (label, e_ln)
        assert e_ph <= 100 * dev_ph, (label, e_ph, dev_ph)
    if name == "small":
        assert b64["counts"].tolist() == [1, 63, 64, 65, 0, 25, 39, 0, 82]
    else:
        assert b64["counts"].tolist() == [141, 145, 148, 149, 149, 149]


# ---- the noise model from warped rows
@pytest.fixture(scope="module")
def noise_cases():
    """{p: (noise model of 9 frames, poles of modulus <= 0.7, silent first, in the middle and last; its model rows at
    Q = 63; the way back on the linear axis in float64 and np.longdouble)}."""
    out = {}
    for p in (2, 18, 50):
        sigma, refl, _ = NR.pole_frames(9, p, 0.7, seed=1, silent=(0, 4, 8))
        C = NR.cepstrum(sigma, refl, 63)
        out[p] = (NR.noise_model(sigma, refl), C, NR.from_cepstrum(C, p), NR.from_cepstrum(C, p, LD))
    return out


@pytest.mark.parametrize("a", [0.42, -0.3])
def test_noise_from_warped_rows(amd, noise_cases, a):
    for p, (nz, C, lin64, linld) in noise_cases.items():
        rows = amd.noise_cepstrum(nz, 63)
        moved = amd.cepstrum_rewarp(rows, 0.0, a, 63)
        got = amd.noise_from_cepstrum(moved, 80, 16000, order=p, cep_warp=a)
        plain = amd.noise_from_cepstrum(rows, 80, 16000, order=p)
        live = lin64[0] > 0
        assert np.array_equal(got["sigma"] == 0, ~live) and np.all(got["refl"][~live] == 0)
        smax = float(lin64[0].max())
        # against the model of the warped route on the same rows: the 100 x rule
        w64, wld = W.noise_from_cepstrum(moved, p, a), W.noise_from_cepstrum(moved, p, a, LD)
        assert not w64[2].any() and not wld[2].any()
        dev_k, dev_s = float(np.abs(w64[1] - wld[1]).max()), float(np.abs(w64[0] - wld[0]).max() / smax)
        err_k = float(np.abs(got["refl"] - w64[1]).max())
        err_s = float(np.abs(got["sigma"] - w64[0]).max() / smax)
        # against the linear route: that rule plus the tail the order-63 cut on the warped axis drops
        full = np.where(np.isneginf(rows), 0.0, rows).astype(LD) @ W.rewarp_matrix(a, 63, 255).T
        tail = 2 * np.abs(full[:, 64:]).sum(axis=1).astype(np.float64)
        lin_k, lin_s = float(np.abs(lin64[1] - linld[1]).max()), float(np.abs(lin64[0] - linld[0]).max() / smax)
        d_k = np.abs(got["refl"] - plain["refl"]).max(axis=1)
        d_s = np.abs(got["sigma"] - plain["sigma"]) / smax
        print("warped noise p %d a %g: k: model dev %.3g gpu err %.3g  sigma: model dev %.3g gpu err %.3g; against the "
              "linear route k %.3g sigma %.3g, tail %.3g" % (p, a, dev_k, err_k, dev_s, err_s, d_k.max(), d_s.max(), tail.max()))
        record_measurement("cepwarp_noise_p%d_a%g" % (p, a), model_dev_k=dev_k, gpu_err_k=err_k, model_dev_sigma=dev_s,
                           gpu_err_sigma=err_s, refl_vs_linear=float(d_k.max()), sigma_vs_linear=float(d_s.max()),
                           tail=float(tail.max()))
        assert err_k <= 100 * dev_k and err_s <= 100 * dev_s, (p, a, err_k, dev_k, err_s, dev_s)
        assert np.all(d_k <= 100 * lin_k + tail) and np.all(d_s <= 100 * lin_s + tail), (p, a, d_k, d_s, tail)


# ---- a cross-check that does not lean on the model
def _geometric_rows(n=5, P=20, r=0.5):
    signs = np.where((np.arange(P + 1)[None, :] * (np.arange(n)[:, None] + 2)) % 3 == 0, -1.0, 1.0)
    C = signs * r ** np.arange(P + 1)[None, :]
    C[:, 0] = -4.0 + 0.5 * np.arange(n)
    return C


@pytest.mark.parametrize("a", [0.42, -0.3, 0.6])
def test_rewarped_rows_read_as_the_linear_ones(amd, a):
    """Rows on the linear axis (P = 20, c_p falling off as 0.5^p with fixed signs), moved to the axis a at order 63 on
    the host: the warped readout of the moved rows is the linear readout of the rows, within the tail the cut drops
    (2 sum_{p > 63} |c~_p| from the order-255 transform) plus the bars of the two readouts."""
    fs = 16000
    C = _geometric_rows()
    moved = amd.cepstrum_rewarp(C, 0.0, a, 63)
    full = C.astype(LD) @ W.rewarp_matrix(a, 20, 255).T
    tail = 2 * np.abs(full[:, 64:]).sum(axis=1).astype(np.float64)
    f = np.linspace(0.0, 0.6 * fs, 61)
    bar = tail + 1e-12 * (_scale_of(C) + _scale_of(moved))
    for what, fn in (("envelope", amd.cepstrum_envelope), ("phase", amd.cepstrum_phase)):
        err = np.abs(fn(moved, fs, f, cep_warp=a) - fn(C, fs, f)).max(axis=1)
        print("rewarped %s a %g: worst difference %.3g, tail %.3g" % (what, a, err.max(), tail.max()))
        record_measurement("cepwarp_rewarp_%s_a%g" % (what, a), difference=float(err.max()), tail=float(tail.max()))
        assert np.all(err <= bar), (what, a, err, bar)


# ---- the round trip of a fit
def test_round_trip_of_a_warped_fit(amd):
    """model_parameters(cep_warp=a), then model_from_parameters(cep_warp=a): the voiced set and f0 come back.  The refit
    of the rebuilt model is recorded, not asserted, as in test_gpu_model_build: the regularised fit on other nodes is not
    an identity."""
    det, fs, _ = other_model()
    a, P, lam = 0.42, 24, 5e-4
    p = amd.model_parameters(det, fs, P, lam, cep_warp=a)
    assert p["cep_warp"] == a and p["voiced"].tolist() == [True] * 7 + [False, True]
    assert p["ceps"].shape == (9, P + 1) and np.isneginf(p["ceps"][7, 0])
    assert np.array_equal(p["ceps"], amd.model_cepstrum(det, fs, P, lam, cep_warp=a))
    built = amd.model_from_parameters(p["f0"], p["ceps"], p["fs"], p["step"], voiced=p["voiced"], cep_warp=p["cep_warp"])
    v = p["voiced"]
    assert np.array_equal((built["amplitudes"] != 0).any(axis=1), v)
    assert np.array_equal(amd.model_parameters(built, fs, P, lam, cep_warp=a)["voiced"], v)
    f0 = amd.model_f0(built, fs)
    assert np.abs(f0[v] / p["f0"][v] - 1).max() <= 1e-12
    back = amd.model_cepstrum(built, fs, P, lam, cep_warp=a)
    diff = float(np.abs(back[v] - p["ceps"][v]).max())
    grid = np.linspace(300.0, 3700.0, 60)
    env = float(np.abs(amd.cepstrum_envelope(back[v], fs, grid, cep_warp=a)
                       - amd.cepstrum_envelope(p["ceps"][v], fs, grid, cep_warp=a)).max())
    print("warped round trip: refit coefficients off by %.3g, envelope by %.3g neper" % (diff, env))
    record_measurement("cepwarp_round_trip", coefficient_difference=diff, envelope_difference=env)


# ---- the entry points' own checks
def test_entry_points_reject_a_bad_warp(amd):
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)

    def z(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=c.device)

    n, K, P, F = 9, 5, 6, 7
    rec, beta, amp, ceps, fr, out = z(n, 3 * K + 1), z(n) + 1.25, z(n, K) - 1.0, z(n, P + 1), z(F), z(n, F)
    f0, th, a0, brec = z(n) + 500.0, z(n), z(n), z(n, 3 * K + 1)
    v = torch.ones(n, dtype=torch.uint8, device=c.device)
    sg, rf = z(n), z(n, 4)
    calls = [lambda a: c.model_cepstrum_warped(rec, n, K, 16000.0, P, 5e-4, ceps, a),
             lambda a: c.modify_amp_cepstrum_warped(rec, n, K, 16000.0, beta, ceps, P, amp, a),
             lambda a: c.cepstrum_envelope_warped(ceps, n, P, 16000.0, fr, F, out, a),
             lambda a: c.cepstrum_phase_warped(ceps, n, P, 16000.0, fr, F, out, a),
             lambda a: c.model_build_warped(f0, th, v, ceps, P, a0, n, 16000.0, K, 1706, False, brec, a),
             lambda a: c.noise_from_cepstrum_warped(ceps, n, P, 4, sg, rf, a)]
    for call in calls:
        for a in (0.0, 0.9, -0.9):
            call(a)                                                     # the good calls, on an empty model
        c.sync()
        for a in (0.9000001, -0.91, float("nan"), float("inf")):
            with pytest.raises(RuntimeError, match="error -1.*cep_warp"):
                call(a)
    with pytest.raises(RuntimeError, match="error -1"):                 # the sibling's checks still hold
        c.model_cepstrum_warped(rec, n, K, 16000.0, 64, 5e-4, ceps, 0.42)
    with pytest.raises(RuntimeError, match="error -1"):
        c.cepstrum_envelope_warped(ceps, n, P, 16000.0, fr, 0, out, 0.42)
    assert c.abi_version == 6
