"""The discrete-cepstrum envelope on the MI355X (model_cepstrum -> eaqhm_model_cepstrum, cepstrum_envelope ->
eaqhm_cepstrum_envelope, eaQHMSynthesis(envelope=...) -> eaqhm_modify_amp_cepstrum) against the NumPy model of
DESIGN.md §9.5 (tests/model_cepstrum_ref.py).  Hand-built models only: no analysis runs.

Bars.  Fit: §10's rule, per case at most 100 x the largest coefficient difference between the model's fit in float64
and in np.longdouble on the same input, computed when the test runs; no instant is left out.  Readout and amplitudes:
the same rule, 100 x the largest difference between the model's readout in float64 and in np.longdouble on the call,
absolute in log amplitude and relative in amplitude (on these cases about 50 times tighter than the fixed
1e-12 x (|c_0| + 2 sum |c_p|) it replaces, which the round trip below still carries as one of its three terms).
Synthesis: 1e-8 of the peak, the bar of test_gpu_model_synthesis and test_gpu_model_formant."""
import numpy as np
import pytest

import model_cepstrum_ref as CR
import model_formant_ref as MF
import model_shape_ref as MS
import model_synthesis_ref as M
from conftest import record_measurement

pytestmark = pytest.mark.gpu

HAND_X = np.array([1000.0, 3000.0, 6000.0])      # the hand map of test_gpu_formant_warp
HAND_Y = np.array([1200.0, 3500.0, 6400.0])
LAMS = (5e-4, 1e-6)


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


def _det(ti, am, fm, ph, a0):
    return dict(ti=ti, isVoiced=np.ones(len(ti), bool), a0=a0, amplitudes=am, frange=fm, pk=ph)


def small_model():
    """9 instants (not a multiple of the 4 waves of a block), Kmax 5, step 80 at 16 kHz.  Slots at 400, 2800, 3000,
    3000 (tied in frequency) and 7000 Hz; instant 4 has no active partial, instant 8 a single node (slot 1), slot 0 is
    missing at instant 6.  (The single node is the last instant: the NumPy synthesis model pads a run of fewer than four
    knots with the first instants, as the reference does, so such a run must not start among them.)"""
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
    """The model the supplied envelopes come from: 9 instants like small_model, but Kmax 12 and harmonics of 310 Hz
    (none of small_model's frequencies); instant 7 has no active partial, so its row is the empty envelope."""
    det, fs, L = harmonic_model(9, 12, 310.0, 16000, jitter=0.01)
    det["amplitudes"][7] = 0.0
    return det, fs, L


def _records(det):
    from eaqhm_amd.model import unpack_model
    m = unpack_model(det)
    return m["records"], m["Kmax"], m["step"]


_REF = {}


def reference_fit(name, det, fs, P, lam):
    """(float64 fit, np.longdouble fit, their largest coefficient difference): computed once per case and shared."""
    key = (name, P, lam)
    if key not in _REF:
        rec = _records(det)[0]
        c64, cld = CR.fit(rec, fs, P, lam), CR.fit(rec, fs, P, lam, np.longdouble)
        fin = np.isfinite(c64)
        assert np.array_equal(fin, np.isfinite(cld))
        _REF[key] = (c64, cld, float(np.abs(c64[fin] - cld[fin]).max()))
    return _REF[key]


def _check_fit(amd, name, det, fs, P, lam):
    rec, K, _ = _records(det)
    got = amd.model_cepstrum(det, fs, P, lam)
    c64, cld, dev = reference_fit(name, det, fs, P, lam)
    assert got.shape == c64.shape == (len(rec), P + 1) and got.dtype == np.float64
    empty = ~((rec[:, :K] != 0) & (rec[:, K:2 * K] > 0)).any(axis=1)
    assert np.all(np.isneginf(got[empty, 0])) and np.all(got[empty, 1:] == 0)          # exactly (-inf, 0, .., 0)
    assert np.all(np.isfinite(got[~empty]))
    err = float(np.abs(got[~empty] - c64[~empty]).max())                                # every non-empty instant
    # the normal equations, taken in np.longdouble: an error within the bar moves G c by at most |G|_inf times it
    worst = 0.0
    for i in np.flatnonzero(~empty):
        G, b = CR.system(*CR.nodes(rec[i, :K], rec[i, K:2 * K], fs, np.longdouble), P, lam, np.longdouble)
        worst = max(worst, float(np.abs(G @ got[i].astype(np.longdouble) - b).max() / np.abs(G).sum(axis=1).max()))
    print("cepstrum fit %s P %d lam %g: model dev %.3g gpu err %.3g (bar %.3g) normal equations %.3g"
          % (name, P, lam, dev, err, 100 * dev, worst))
    record_measurement("cepstrum_fit_vs_numpy_%s_P%d_lam%g" % (name, P, lam), model_dev=dev, gpu_err=err,
                       bar=100 * dev, normal_equations=worst)
    assert dev > 0
    assert err <= 100 * dev, (name, P, lam, err, dev)
    assert worst <= 100 * dev, (name, P, lam, worst, dev)
    return got


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("P", [1, 5, 63])
def test_fit_small(amd, P, lam):
    """P = 5 and 63: more coefficients than the instants have nodes (5 at most, 1 at instant 8)."""
    det, fs, _ = small_model()
    got = _check_fit(amd, "small", det, fs, P, lam)
    assert np.isneginf(got[4, 0]) and np.all(np.isfinite(got[[8, 6]]))


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("P", [50, 63])
def test_fit_wide(amd, P, lam):
    det, fs, _ = wide_model()
    assert np.asarray(det["amplitudes"]).shape[1] == 148
    _check_fit(amd, "wide", det, fs, P, lam)


def test_fit_default_order_and_other_model(amd):
    det, fs, _ = other_model()
    got = amd.model_cepstrum(det, fs)
    assert got.shape == (9, 19)                                  # min(63, 2 + round(16000 / 1000)) = 18
    c64, _, dev = reference_fit("other", det, fs, 18, 5e-4)
    keep = np.r_[0:7, 8]
    assert np.isneginf(got[7, 0]) and np.all(got[7, 1:] == 0)
    assert np.abs(got[keep] - c64[keep]).max() <= 100 * dev


@pytest.mark.parametrize("P,lam", [(5, 5e-4), (63, 1e-6)])
def test_constant_on_ln_am_moves_c0_alone_on_the_gpu(amd, P, lam):
    """am times e^s: c_0 moves by s, the others stay.  Each of the two fits is within its own bar of its model, and the
    two models differ by the shift up to their own deviation: the sum of the two bars."""
    det, fs, _ = small_model()
    s = 1.75
    moved = dict(det, amplitudes=det["amplitudes"] * np.exp(s))
    a, b = amd.model_cepstrum(det, fs, P, lam), amd.model_cepstrum(moved, fs, P, lam)
    bar = 100 * (reference_fit("small", det, fs, P, lam)[2] + reference_fit("small_moved", moved, fs, P, lam)[2])
    keep = np.r_[0:4, 5:9]
    d0 = float(np.abs((b[keep, 0] - a[keep, 0]) - s).max())
    dp = float(np.abs(b[keep, 1:] - a[keep, 1:]).max())
    record_measurement("cepstrum_fit_shift_P%d_lam%g" % (P, lam), c0_error=d0, others=dp, bar=bar)
    assert d0 <= bar and dp <= bar, (d0, dp, bar)
    assert np.isneginf(b[4, 0])


def _readout_bar(C):
    return 1e-12 * (np.abs(C[:, 0]) + 2 * np.abs(C[:, 1:]).sum(axis=1))


def _check_readout(amd, label, C, fs, grid, alpha=None, warp=None):
    kw = {}
    if alpha is not None:
        kw["formant_scale"] = alpha
    if warp is not None:
        kw["formant_warp"] = warp
    got = amd.cepstrum_envelope(C, fs, grid, **kw)
    ref = CR.envelope(C, fs, grid, alpha, warp)
    assert got.shape == ref.shape == (len(C), len(grid)) and got.dtype == np.float64
    empty = np.isneginf(C[:, 0])
    assert np.all(np.isneginf(got[empty])) and np.all(np.isfinite(got[~empty]))
    dev = float(np.abs(ref[~empty] - CR.envelope(C, fs, grid, alpha, warp, np.longdouble)[~empty]).max())
    err = float(np.abs(got[~empty] - ref[~empty]).max())
    print("cepstrum readout %s: model dev %.3g gpu err %.3g" % (label, dev, err))
    record_measurement("cepstrum_readout_vs_numpy_%s" % label, model_dev=dev, gpu_err=err,
                       worst_error_over_bar=err / (100 * dev))
    assert dev > 0 and err <= 100 * dev, (label, err, dev)
    return got


def test_readout_against_numpy(amd):
    """33 points from 0 to 0.6 fs: the hold past fs/2 is on the grid."""
    det, fs, _ = other_model()
    C = reference_fit("other", det, fs, 18, 5e-4)[0]
    assert np.isneginf(C[7, 0])
    n = len(C)
    grid = np.linspace(0.0, 0.6 * fs, 33)
    plain = _check_readout(amd, "plain", C, fs, grid)
    past = grid >= fs / 2
    at = amd.cepstrum_envelope(C, fs, [fs / 2.0])
    assert past.sum() > 1 and np.array_equal(plain[:, past], np.repeat(at, past.sum(), axis=1))     # held
    _check_readout(amd, "alpha0.85", C, fs, grid, alpha=0.85)
    _check_readout(amd, "alpha_rows", C, fs, grid, alpha=np.linspace(0.8, 1.25, n))
    _check_readout(amd, "hand_map", C, fs, grid, warp=(HAND_X, HAND_Y))
    _check_readout(amd, "hand_map_rows", C, fs, grid,
                   warp=(HAND_X, HAND_Y[None, :] * (1.0 + 0.01 * np.arange(n))[:, None]))
    _check_readout(amd, "b1", C, fs, grid, warp=(np.array([1000.0]), np.array([1180.0])))
    assert np.array_equal(amd.cepstrum_envelope(C, fs, grid, formant_warp=(HAND_X, HAND_X.copy())), plain)
    assert np.array_equal(amd.cepstrum_envelope(C, fs, grid, 1.0), plain)
    # the highest order, at 48 kHz
    det, fs, _ = wide_model()
    C = reference_fit("wide", det, fs, 63, 5e-4)[0]
    _check_readout(amd, "wide_P63", C, fs, np.linspace(0.0, 0.6 * fs, 33))
    _check_readout(amd, "wide_P63_alpha1.2", C, fs, np.linspace(0.0, 0.6 * fs, 33), alpha=1.2)


def test_amplitudes_from_another_models_cepstrum(amd):
    """Context.modify_amp_cepstrum on device tensors after a prep without the envelope.  The cepstra come from
    other_model (Kmax 12, harmonics of 310 Hz) and are read at small_model's slots (Kmax 5)."""
    import torch
    from eaqhm_amd.functions import _ctx
    det, fs, _ = small_model()
    rec_h, K, D = _records(det)
    n = len(rec_h)
    odet, ofs, _ = other_model()
    C = reference_fit("other", odet, ofs, 18, 5e-4)[0]
    P = C.shape[1] - 1
    am, fm = rec_h[:, :K], rec_h[:, K:2 * K]
    c = _ctx(0)
    dev = c.device

    def t(x):
        return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)

    rec, C_d = t(rec_h), t(C)
    code = torch.empty(n * K, dtype=torch.uint8, device=dev)
    mom = torch.empty(n * (K + 1), dtype=torch.float64, device=dev)
    c.spline_solve(rec, n, K, D, code, mom)
    rows = np.tile(HAND_Y, (n, 1))
    cases = [("beta1", 1.0, None, None), ("beta1.25", 1.25, None, None), ("beta1.25_alpha1.2", 1.25, 1.2, None),
             ("beta1_alpha1.2", 1.0, 1.2, None), ("beta1_hand", 1.0, None, (HAND_X, rows)),
             ("beta1.25_hand", 1.25, None, (HAND_X, rows))]
    for label, beta, alpha, warp in cases:
        beta_d = t(np.full(n, beta))
        amp, R, ph0 = (torch.full((n, K), -1.0, dtype=torch.float64, device=dev) for _ in range(3))
        c.modify_prep(rec, code, mom, n, K, D, float(fs), beta_d, None, None, False, amp, R, ph0)
        c.modify_amp_cepstrum(rec, n, K, float(fs), beta_d, C_d, P, amp,
                              alpha=None if alpha is None else t(np.full(n, alpha)),
                              warp=None if warp is None else (t(warp[0]), t(warp[1]), len(warp[0])))
        got = amp.cpu().numpy()
        ref = CR.amplitudes(am, fm, fs, beta, C, alpha, warp)
        active = (am != 0) & (fm > 0)
        zero = ~active | (beta * fm >= fs / 2) | np.isneginf(C[:, :1])
        assert np.array_equal(ref == 0, zero)
        assert np.array_equal(got == 0, zero), label          # exactly 0: inactive, past Nyquist, the empty row
        assert np.all(got[4] == 0) and got[6, 0] == 0 and np.all(got[7] == 0)
        if beta == 1.25:
            assert np.all(got[:, 4] == 0)                      # 8750 Hz
        ref_l = CR.amplitudes(am, fm, fs, beta, C, alpha, warp, np.longdouble)
        mdev = float(np.abs(ref_l[~zero] / ref[~zero] - 1.0).max())
        err = float(np.abs(got[~zero] / ref[~zero] - 1.0).max())
        print("cepstrum amplitudes %s: model dev %.3g gpu err %.3g" % (label, mdev, err))
        record_measurement("cepstrum_amplitudes_vs_numpy_%s" % label, model_dev=mdev, gpu_err=err,
                           worst_error_over_bar=err / (100 * mdev))
        assert mdev > 0 and err <= 100 * mdev, (label, err, mdev)
        if beta == 1.0 and alpha is None and warp is None:
            assert not np.array_equal(got, am)                 # no unit rule: the amplitudes are the envelope's


SYNTH_CASES = [("plain", {}, {}), ("alpha1.2", dict(formant_scale=1.2), dict(alpha=1.2)),
               ("hand", dict(formant_warp=(HAND_X, HAND_Y)), dict(warp=(HAND_X, HAND_Y))),
               ("shape", dict(phase="shape"), {})]


@pytest.mark.parametrize("rho,beta", [(1.0, 1.0), (0.5, 1.25)])
def test_synthesis_with_a_supplied_envelope(amd, rho, beta):
    det, fs, L = small_model()
    rec, K, D = _records(det)
    odet, ofs, _ = other_model()
    C = reference_fit("other", odet, ofs, 18, 5e-4)[0]
    for label, kw, rkw in SYNTH_CASES:
        out = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, envelope=C, **kw)
        Ap = CR.amplitudes(rec[:, :K], rec[:, K:2 * K], fs, beta, C, **rkw)
        with MF._amplitudes(Ap):
            if label == "shape":
                ref = MS.synthesize_shape(rec, D, fs, L, rho, beta)
            else:
                ref = M.synthesize(rec, D, fs, L, rho, beta, True)
        assert out.shape == ref.shape == (int(np.rint(rho * L)),) and out.dtype == np.float64
        rel = float(np.abs(out - ref).max() / np.abs(ref).max())
        print("cepstrum synthesis %s rho %g beta %g: max rel %.3g" % (label, rho, beta, rel))
        record_measurement("cepstrum_synthesis_vs_numpy_%s_rho%g_beta%g" % (label, rho, beta), max_rel=rel)
        assert rel <= 1e-8, (label, rho, beta, rel)
        n1, n2 = len(out) // 3, 2 * len(out) // 3 + 7
        parts = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, envelope=C,
                                   _ranges=[(0, n1), (n1, n2), (n2, len(out))], **kw)
        assert np.array_equal(parts, out), (label, rho, beta)
        if label == "plain":      # the envelope is the caller's: not the model's own amplitudes, not even at unit scales
            assert not np.array_equal(out, amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta))


def test_synthesis_with_a_contour_and_the_models_own_fit(amd):
    """A contour of rho selects the contour path; the envelope is the GPU's own fit of the same model."""
    import model_contour_ref as MC
    det, fs, L = small_model()
    rec, K, D = _records(det)
    n = len(rec)
    C = amd.model_cepstrum(det, fs, 8, 5e-4)
    rho = np.linspace(0.8, 1.4, n)
    out = amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=1.25, envelope=C)
    Ap = CR.amplitudes(rec[:, :K], rec[:, K:2 * K], fs, 1.25, C)
    with MF._amplitudes(Ap):
        ref = MC.synthesize_contour(rec, D, fs, L, rho.copy(), np.full(n, 1.25), True)
    assert out.shape == ref.shape
    rel = float(np.abs(out - ref).max() / np.abs(ref).max())
    record_measurement("cepstrum_synthesis_vs_numpy_contour", max_rel=rel)
    assert rel <= 1e-8, rel


def test_round_trip_of_a_known_cepstral_curve(amd):
    """ln am are samples of a known order-8 curve at 40 harmonics of 180 Hz: model_cepstrum at P = 8, lam = 1e-6, then
    cepstrum_envelope at the partial frequencies, returns ln am.  Bar: what the model's own fit leaves on that input
    (the bias of the regulariser, measured here), plus the fit bar carried through the readout (an error e in every
    coefficient moves the envelope by at most (1 + 2 P) e), plus the readout bar."""
    fs, P, lam, n, K = 16000, 8, 1e-6, 5, 40
    ti = np.arange(n) * 80
    rng = np.random.default_rng(5)
    true = np.concatenate((-4.0 + 0.2 * rng.standard_normal((n, 1)),
                           rng.standard_normal((n, P)) / (1.0 + np.arange(1, P + 1)) ** 1.5), axis=1)
    fm = np.tile(180.0 * np.arange(1, K + 1), (n, 1))
    lna = CR.readout(true, fs, fm)
    det = _det(ti, np.exp(lna), fm, np.zeros((n, K)), np.zeros(n))
    c64, _, dev = reference_fit("roundtrip", det, fs, P, lam)
    bias = float(np.abs(CR.readout(c64, fs, fm) - lna).max())
    C = amd.model_cepstrum(det, fs, P, lam)
    back = np.stack([amd.cepstrum_envelope(C[i:i + 1], fs, fm[i])[0] for i in range(n)])
    err = float(np.abs(back - lna).max())
    bar = bias + (1 + 2 * P) * 100 * dev + float(_readout_bar(C).max())
    print("cepstrum round trip: bias of the model's fit %.3g, gpu error %.3g, bar %.3g; coefficients off by %.3g"
          % (bias, err, bar, float(np.abs(C - true).max())))
    record_measurement("cepstrum_round_trip", model_bias=bias, model_dev=dev, gpu_err=err, bar=bar,
                       coefficient_error=float(np.abs(C - true).max()))
    assert err <= bar, (err, bar)
    assert bias <= 1e-3                                        # the curve is in the basis: only lam keeps it off


def test_entry_points_reject_bad_arguments(amd):
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)

    def z(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=c.device)

    n, K, P, F, B = 9, 5, 6, 7, 2
    rec, beta, amp, ceps, fr, out, al = z(n, 3 * K + 1), z(n) + 1.25, z(n, K) - 1.0, z(n, P + 1), z(F), z(n, F), z(n) + 1.1
    x = torch.as_tensor(np.array([1000.0, 4000.0]), device=c.device)
    y = torch.as_tensor(np.tile([1100.0, 4000.0], (n, 1)), device=c.device)
    c.model_cepstrum(rec, n, K, 16000.0, P, 5e-4, ceps)             # the good calls, on an empty model
    c.sync()
    assert torch.all(torch.isinf(ceps[:, 0])) and torch.all(ceps[:, 1:] == 0)
    for kw in (dict(), dict(alpha=al), dict(warp=(x, y, B))):
        c.modify_amp_cepstrum(rec, n, K, 16000.0, beta, ceps, P, amp, **kw)
        c.cepstrum_envelope(ceps, n, P, 16000.0, fr, F, out, **kw)
        c.sync()
        assert torch.all(amp == 0) and torch.all(torch.isinf(out))
    c.model_cepstrum(rec, 1, K, 16000.0, P, 5e-4, ceps)              # a single instant is a model for the fit

    def bad(fn, *a, **k):
        with pytest.raises(RuntimeError, match="error -1"):
            fn(*a, **k)

    for order in (0, 64, -1):
        bad(c.model_cepstrum, rec, n, K, 16000.0, order, 5e-4, ceps)
        bad(c.modify_amp_cepstrum, rec, n, K, 16000.0, beta, ceps, order, amp)
        bad(c.cepstrum_envelope, ceps, n, order, 16000.0, fr, F, out)
    for lam in (0.0, -1e-3, float("nan"), float("inf")):
        bad(c.model_cepstrum, rec, n, K, 16000.0, P, lam, ceps)
    bad(c.model_cepstrum, rec, 0, K, 16000.0, P, 5e-4, ceps)
    bad(c.model_cepstrum, rec, n, 0, 16000.0, P, 5e-4, ceps)
    bad(c.model_cepstrum, rec, n, K, 0.0, P, 5e-4, ceps)
    bad(c.model_cepstrum, rec, n, 100000, 16000.0, P, 5e-4, ceps)       # Kmax beyond the LDS budget of the fit
    bad(c.model_cepstrum, None, n, K, 16000.0, P, 5e-4, ceps)
    bad(c.model_cepstrum, rec, n, K, 16000.0, P, 5e-4, None)
    bad(c.modify_amp_cepstrum, rec, 3, K, 16000.0, beta, ceps, P, amp)
    bad(c.modify_amp_cepstrum, rec, n, K, float("nan"), beta, ceps, P, amp)
    bad(c.cepstrum_envelope, ceps, 0, P, 16000.0, fr, F, out)
    bad(c.cepstrum_envelope, ceps, n, P, 16000.0, fr, 0, out)
    for j in (0, 4, 5, 7):       # records, beta, ceps, amp
        args = [rec, n, K, 16000.0, beta, ceps, P, amp]
        args[j] = None
        bad(c.modify_amp_cepstrum, *args)
    for j in (0, 4, 6):          # ceps, freqs, out
        args = [ceps, n, P, 16000.0, fr, F, out]
        args[j] = None
        bad(c.cepstrum_envelope, *args)
    for warp in ((x, y, 0), (x, y, 17), (x, y, -1), (x, None, B), (None, y, B), (None, None, B)):
        bad(c.modify_amp_cepstrum, rec, n, K, 16000.0, beta, ceps, P, amp, warp=warp)
        bad(c.cepstrum_envelope, ceps, n, P, 16000.0, fr, F, out, warp=warp)
    bad(c.modify_amp_cepstrum, rec, n, K, 16000.0, beta, ceps, P, amp, alpha=al, warp=(x, y, B))
    bad(c.cepstrum_envelope, ceps, n, P, 16000.0, fr, F, out, alpha=al, warp=(x, y, B))
    assert c.abi_version == 6
