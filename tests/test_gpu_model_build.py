"""A harmonic model from f0 and cepstral rows on the MI355X (model_from_parameters -> eaqhm_model_build,
cepstrum_phase -> eaqhm_cepstrum_phase) against the NumPy model of DESIGN.md §9.7 (tests/model_build_ref.py).
Hand-built parameters only: no analysis runs.

Bars.  Active set, frequencies and the zeros of inactive cells: exact.  ln |a|: §9.5's readout bar, 1e-12 x
(|c_0| + 2 sum |c_p|) per row.  Phases, mod 2 pi: §10's rule, per case at most 100 x the largest difference between the
model in float64 and in np.longdouble on the same input, computed when the test runs; no cell is left out.
cepstrum_phase: the readout bar.  Synthesis: 1e-8 of the peak, the bar of test_gpu_model_synthesis and
test_gpu_model_shape."""
import numpy as np
import pytest

import model_build_ref as MB
import model_cepstrum_ref as CR
import model_shape_ref as MS
import model_synthesis_ref as M
from conftest import record_measurement

pytestmark = pytest.mark.gpu

HAND_X = np.array([1000.0, 3000.0, 6000.0])      # the hand map of test_gpu_formant_warp
HAND_Y = np.array([1200.0, 3500.0, 6400.0])


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


def _rows(n, P, seed):
    """Formant-like rows: c_0 about -4, coefficients falling off with p."""
    rng = np.random.default_rng(seed)
    return np.concatenate((-4.0 + 0.3 * rng.standard_normal((n, 1)),
                           rng.standard_normal((n, P)) / (1.0 + np.arange(1, P + 1)) ** 1.2), axis=1)


def small(P):
    """9 instants (not a multiple of the 4 waves of a block) at 16 kHz, step 80: 1, 63, 64, 65, -, 25, 39, -, 82
    harmonics (a lane-chunk boundary, rows shorter than Kmax); instant 4 is unvoiced, instant 7 an empty row.  Runs of
    fewer than four knots do not start among the first instants (the NumPy synthesis pads them with those)."""
    f0 = np.array([5000.0, 125.0, 124.0, 123.0, 150.0, 310.0, 200.0, 180.0, 97.5])
    voiced = np.ones(9, bool)
    voiced[4] = False
    C = _rows(9, P, 11 + P)
    C[7] = 0.0
    C[7, 0] = -np.inf
    return dict(f0=f0, voiced=voiced, ceps=C, fs=16000, step=80, theta0=0.3, a0=0.001 * np.arange(9) * voiced)


def wide(P):
    """6 instants at 48 kHz, step 240: 141 to 149 harmonics (160 Hz), three lane chunks."""
    f0 = np.array([170.0, 165.0, 162.0, 161.0, 160.0, 160.0])
    return dict(f0=f0, voiced=np.ones(6, bool), ceps=_rows(6, P, 5 + P), fs=48000, step=240, theta0=0.0, a0=None)


CASES = {"small": small, "wide": wide}
_REF = {}


def reference(name, P, kmax=None, zero=False):
    """(parameters, the model in float64, the model in np.longdouble, their largest phase difference mod 2 pi over the
    active cells): computed once per case and shared."""
    key = (name, P, kmax, zero)
    if key not in _REF:
        p = CASES[name](P)
        kw = dict(theta0=p["theta0"], kmax=kmax, a0=p["a0"], zero_phase=zero)
        b64 = MB.build(p["f0"], p["voiced"], p["ceps"], p["fs"], p["step"], **kw)
        bld = MB.build(p["f0"], p["voiced"], p["ceps"], p["fs"], p["step"], dtype=np.longdouble, **kw)
        assert np.array_equal(b64["active"], bld["active"])
        d = (bld["phase"] - b64["phase"].astype(np.longdouble)).astype(np.float64)
        dev = float(np.abs(np.angle(np.exp(1j * d)))[b64["active"]].max())
        _REF[key] = (p, b64, bld, dev)
    return _REF[key]


def _build(amd, p, kmax=None, phase="minimum"):
    return amd.model_from_parameters(p["f0"], p["ceps"], p["fs"], p["step"], voiced=p["voiced"], phase=phase,
                                     theta0=p["theta0"], kmax=kmax, a0=p["a0"])


def _readout_bar(C):
    c0 = np.where(np.isfinite(C[:, 0]), C[:, 0], 0.0)
    return 1e-12 * (np.abs(c0) + 2 * np.abs(C[:, 1:]).sum(axis=1))


def _mod(d):
    return np.abs(np.angle(np.exp(1j * d)))


def _check_records(amd, name, P, kmax=None):
    p, b64, _, dev = reference(name, P, kmax)
    det = _build(amd, p, kmax)
    n, K = len(p["f0"]), b64["Kmax"]
    rec, act = b64["records"], b64["active"]
    am, fm, pk = det["amplitudes"], det["frange"], det["pk"]
    assert am.shape == fm.shape == pk.shape == (n, K) and am.dtype == np.float64
    assert np.array_equal(det["ti"], np.arange(n) * p["step"]) and np.array_equal(det["isVoiced"], p["voiced"])
    assert np.array_equal(det["a0"], rec[:, 3 * K])
    assert np.array_equal(am != 0, act)                                         # the active set, exactly
    assert np.array_equal(fm, rec[:, K:2 * K])                                  # h * f0, and 0 where inactive
    assert np.all(pk[~act] == 0) and np.all(np.abs(pk) <= np.pi)
    bar = np.broadcast_to(_readout_bar(p["ceps"])[:, None], (n, K))
    e_ln = np.abs(np.log(am[act]) - b64["lnam"][act]) / bar[act]                # every active cell
    e_ph = _mod(pk - rec[:, 2 * K:3 * K])[act]
    # the zero-phase model under the same bar
    _, z64, _, _ = reference(name, P, kmax, True)
    zdet = _build(amd, p, kmax, "zero")
    assert np.array_equal(zdet["amplitudes"], am) and np.array_equal(zdet["frange"], fm)
    h = np.arange(1, K + 1)
    assert np.array_equal(z64["active"], act)
    e_z = _mod(zdet["pk"] - z64["records"][:, 2 * K:3 * K])[act]
    assert _mod(z64["records"][:, 2 * K:3 * K] - 2 * np.pi * h[None, :] * z64["theta"][:, None])[act].max() < 1e-11
    label = "%s_P%d%s" % (name, P, "" if kmax is None else "_kmax%d" % kmax)
    print("model build %s: ln am error / bar %.3g; model dev %.3g, phase error %.3g (ratio %.3g), zero-phase %.3g"
          % (label, e_ln.max(), dev, e_ph.max(), e_ph.max() / dev, e_z.max()))
    record_measurement("model_build_vs_numpy_%s" % label, ln_am_error_over_bar=float(e_ln.max()), model_dev=dev,
                       phase_error=float(e_ph.max()), phase_error_over_dev=float(e_ph.max() / dev),
                       zero_phase_error_over_dev=float(e_z.max() / dev))
    assert dev > 0
    assert e_ln.max() <= 1.0, (label, e_ln.max())
    assert e_ph.max() <= 100 * dev, (label, e_ph.max(), dev)
    assert e_z.max() <= 100 * dev, (label, e_z.max(), dev)
    return det, b64


@pytest.mark.parametrize("P", [1, 18, 63])
def test_records_small(amd, P):
    det, b64 = _check_records(amd, "small", P)
    assert b64["counts"].tolist() == [1, 63, 64, 65, 0, 25, 39, 0, 82] and det["amplitudes"].shape[1] == 82
    assert np.all(det["amplitudes"][[4, 7]] == 0) and np.all(det["pk"][[4, 7]] == 0)


@pytest.mark.parametrize("P", [18, 63])
def test_records_wide(amd, P):
    det, b64 = _check_records(amd, "wide", P)
    assert b64["counts"].tolist() == [141, 145, 148, 149, 149, 149]


def test_records_capped(amd):
    det, b64 = _check_records(amd, "small", 18, kmax=40)
    assert b64["counts"].tolist() == [1, 40, 40, 40, 0, 25, 39, 0, 40] and det["amplitudes"].shape[1] == 40
    full = _build(amd, reference("small", 18)[0])
    for key in ("amplitudes", "frange", "pk"):
        assert np.array_equal(det[key], full[key][:, :40])


def test_cepstrum_phase_against_numpy(amd):
    p = small(18)
    C, fs, n = p["ceps"], p["fs"], 9
    grid = np.linspace(0.0, 0.6 * fs, 120)                       # the hold past fs/2 is on the grid
    bar = _readout_bar(C)[:, None]
    cases = [("plain", {}, {}), ("alpha1.18", dict(formant_scale=1.18), dict(alpha=1.18)),
             ("hand_map", dict(formant_warp=(HAND_X, HAND_Y)), dict(warp=(HAND_X, HAND_Y)))]
    for label, kw, rkw in cases:
        got = amd.cepstrum_phase(C, fs, grid, **kw)
        ref = MB.series(np.where(np.isfinite(C), C, 0.0), fs, CR.read_frequency(grid, n, **rkw))[1]
        assert got.shape == ref.shape == (n, len(grid)) and got.dtype == np.float64
        assert np.all(got[7] == 0) and np.all(got[:, 0] == 0)    # the empty row; Phi(0) = 0
        rel = np.delete(np.abs(got - ref), 7, axis=0) / np.delete(bar, 7, axis=0)      # row 7 is the empty row
        print("cepstrum phase %s: worst error / bar %.3g" % (label, rel.max()))
        record_measurement("cepstrum_phase_vs_numpy_%s" % label, worst_error_over_bar=float(rel.max()))
        assert rel.max() <= 1.0, (label, rel.max())
        assert np.abs(got).max() > 0.1
    plain = amd.cepstrum_phase(C, fs, grid)
    past = grid >= fs / 2
    assert past.sum() > 1 and np.array_equal(plain[:, past], np.repeat(amd.cepstrum_phase(C, fs, [fs / 2.0]), past.sum(), 1))
    # P = 63 at 48 kHz
    q = wide(63)
    got = amd.cepstrum_phase(q["ceps"], q["fs"], np.linspace(0.0, 0.6 * q["fs"], 120))
    ref = MB.series(q["ceps"], q["fs"], np.linspace(0.0, 0.6 * q["fs"], 120))[1]
    rel = float((np.abs(got - ref) / _readout_bar(q["ceps"])[:, None]).max())
    record_measurement("cepstrum_phase_vs_numpy_wide_P63", worst_error_over_bar=rel)
    assert rel <= 1.0, rel


def test_the_built_phases_are_the_carrier_plus_cepstrum_phase(amd):
    """At the built model's own frequencies cepstrum_phase agrees with pk - 2 pi frac(h theta) (mod 2 pi) within the sum
    of the two bars; cepstrum_envelope there is ln of the amplitudes; model_f0 returns f0."""
    p, b64, _, dev = reference("small", 18)
    det = _build(amd, p)
    C, fs = p["ceps"], p["fs"]
    act = b64["active"]
    bar = _readout_bar(C)
    worst_p = worst_a = 0.0
    for i in np.flatnonzero(act.any(axis=1)):
        a = act[i]
        phi = amd.cepstrum_phase(C[i:i + 1], fs, det["frange"][i])[0]
        worst_p = max(worst_p, float((_mod(det["pk"][i] - b64["carrier"][i] - phi)[a] / (bar[i] + 100 * dev)).max()))
        env = amd.cepstrum_envelope(C[i:i + 1], fs, det["frange"][i])[0]
        worst_a = max(worst_a, float((np.abs(env[a] - np.log(det["amplitudes"][i][a])) / bar[i]).max()))
    record_measurement("model_build_cross_checks", phase_over_bars=worst_p, envelope_over_bar=worst_a)
    assert worst_p <= 1.0 and worst_a <= 1.0, (worst_p, worst_a)
    f0 = amd.model_f0(det, fs)
    has = act.any(axis=1)
    assert np.abs(f0[has] / p["f0"][has] - 1).max() <= 1e-12
    from eaqhm_amd.model import unpack_model
    assert unpack_model(det)["quirk_cells"] == 0


def test_synthesis_with_the_same_envelope_supplied(amd):
    """envelope=ceps reads the same C at the same frequencies as the build did."""
    p = reference("small", 18)[0]
    det = _build(amd, p)
    L = 8 * p["step"] + 1
    a = amd.eaQHMSynthesis(det, p["fs"], L)
    b = amd.eaQHMSynthesis(det, p["fs"], L, envelope=p["ceps"])
    rel = float(np.abs(a - b).max() / np.abs(a).max())
    record_measurement("model_build_synthesis_envelope_route", max_rel=rel)
    assert rel <= 1e-8 and np.abs(a).max() > 1e-3, rel


@pytest.mark.parametrize("name,P", [("small", 18), ("wide", 63)])
def test_synthesis_against_numpy(amd, name, P):
    p, b64, _, _ = reference(name, P)
    det = _build(amd, p)
    fs, D, rec = p["fs"], p["step"], b64["records"]
    L = (len(rec) - 1) * D + 1
    out = amd.eaQHMSynthesis(det, fs, L)
    ref = M.synthesize(rec, D, fs, L)
    assert out.shape == ref.shape == (L,)
    rel = float(np.abs(out - ref).max() / np.abs(ref).max())
    out_s = amd.eaQHMSynthesis(det, fs, L, time_scale=1.5, pitch_scale=1.2, phase="shape")
    ref_s = MS.synthesize_shape(rec, D, fs, L, 1.5, 1.2)
    assert out_s.shape == ref_s.shape == (int(np.rint(1.5 * L)),)
    rel_s = float(np.abs(out_s - ref_s).max() / np.abs(ref_s).max())
    print("model build synthesis %s: max rel %.3g, scaled with the shape phase %.3g" % (name, rel, rel_s))
    record_measurement("model_build_synthesis_vs_numpy_%s" % name, max_rel=rel, max_rel_shape=rel_s)
    assert rel <= 1e-8 and rel_s <= 1e-8, (name, rel, rel_s)


def harmonic_model(n, K, f0, fs, step=80, jitter=0.0):
    """The hand model of test_gpu_model_cepstrum: n instants of K harmonics of f0 with a formant-shaped ln am."""
    ti = np.arange(n) * step
    k = np.arange(1, K + 1)
    fm = f0 * k[None, :] * (1.0 + jitter * np.sin(0.7 * np.arange(n))[:, None])
    lna = (-3.0 - fm / 5000.0 + 2.0 * np.exp(-((fm - (700.0 + 20.0 * np.arange(n)[:, None])) / 300.0) ** 2)
           + 1.5 * np.exp(-((fm - 2400.0) / 500.0) ** 2) + 0.2 * np.sin(1.3 * k[None, :] + np.arange(n)[:, None]))
    ph = np.angle(np.exp(1j * 2 * np.pi * fm * ti[:, None] / fs))
    return dict(ti=ti, isVoiced=np.ones(n, bool), a0=np.zeros(n), amplitudes=np.exp(lna), frange=fm, pk=ph), fs


def test_round_trip(amd):
    """model_parameters, then model_from_parameters: the voiced set and f0 come back.  The refit of the rebuilt model
    (25 harmonics where the original had 12) is recorded, not asserted: the regularised fit on other nodes is not an
    identity."""
    det, fs = harmonic_model(9, 12, 310.0, 16000, jitter=0.01)
    det["amplitudes"][7] = 0.0
    P, lam = 18, 5e-4
    p = amd.model_parameters(det, fs, P, lam)
    assert p["voiced"].tolist() == [True] * 7 + [False, True] and p["step"] == 80 and p["fs"] == 16000.0
    assert p["ceps"].shape == (9, P + 1) and np.isneginf(p["ceps"][7, 0])
    built = amd.model_from_parameters(p["f0"], p["ceps"], p["fs"], p["step"], voiced=p["voiced"])
    v = p["voiced"]
    assert np.array_equal((built["amplitudes"] != 0).any(axis=1), v)
    assert np.array_equal(amd.model_parameters(built, fs, P, lam)["voiced"], v)
    f0 = amd.model_f0(built, fs)
    assert np.abs(f0[v] / p["f0"][v] - 1).max() <= 1e-12
    back = amd.model_cepstrum(built, fs, P, lam)
    diff = float(np.abs(back[v] - p["ceps"][v]).max())
    grid = np.linspace(300.0, 3700.0, 60)
    env = float(np.abs(amd.cepstrum_envelope(back[v], fs, grid) - amd.cepstrum_envelope(p["ceps"][v], fs, grid)).max())
    print("model build round trip: refit coefficients off by %.3g, envelope by %.3g neper" % (diff, env))
    record_measurement("model_build_round_trip", coefficient_difference=diff, envelope_difference=env)


def test_entry_points_reject_bad_arguments(amd):
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)

    def z(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=c.device)

    n, K, P, F = 5, 7, 6, 3
    f0, th, a0, ceps, rec = z(n) + 500.0, z(n), z(n), z(n, P + 1), z(n, 3 * K + 1) - 1.0
    v = torch.ones(n, dtype=torch.uint8, device=c.device)
    c.model_build(f0, th, v, ceps, P, a0, n, 16000.0, K, 1706, False, rec)          # the good call: C = 0, |a| = 1
    c.sync()
    assert torch.all(rec[:, :K] == 1) and torch.all(rec[:, 2 * K:] == 0)
    assert torch.equal(rec[0, K:2 * K], torch.arange(1, K + 1, device=c.device) * 500.0)

    def bad(fn, *a, **k):
        with pytest.raises(RuntimeError, match="error -1"):
            fn(*a, **k)

    good = [f0, th, v, ceps, P, a0, n, 16000.0, K, 1706, False, rec]
    for j, val in ((0, None), (1, None), (2, None), (3, None), (5, None), (11, None), (4, 0), (4, 64), (6, 1), (6, 0),
                   (7, 0.0), (7, float("nan")), (8, 0), (8, 1707), (9, 0), (9, 1707), (9, K - 1)):
        args = list(good)
        args[j] = val
        bad(c.model_build, *args)
    fr, out = z(F) + 100.0, z(n, F)
    c.cepstrum_phase(ceps, n, P, 16000.0, fr, F, out)
    for order in (0, 64):
        bad(c.cepstrum_phase, ceps, n, order, 16000.0, fr, F, out)
    bad(c.cepstrum_phase, ceps, 0, P, 16000.0, fr, F, out)
    bad(c.cepstrum_phase, ceps, n, P, 16000.0, fr, 0, out)
    bad(c.cepstrum_phase, None, n, P, 16000.0, fr, F, out)
    bad(c.cepstrum_phase, ceps, n, P, 16000.0, fr, F, out, alpha=z(n) + 1.1, warp=(z(2), z(n, 2), 2))
    assert c.abi_version == 6
