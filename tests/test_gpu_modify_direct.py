"""The kernels of csrc/eaqhm_modify.hip (eaqhm_modify_prep_kernel, eaqhm_modify_scan_kernel, eaqhm_modify_carry_kernel
and the four eval kernels) through hip.Context, on the hand-built models of tests/modify_cases.py: spline_solve ->
modify_prep -> modify_synth on device tensors, every output buffer pre-filled with a sentinel, and the intermediate
arrays (code, amp, R, ph0) compared cell by cell with the NumPy model of DESIGN.md §9 (tests/model_synthesis_ref.py)
before the samples are.

Bars, per quantity and per slot, as test_gpu_interp_stage.bar_of: 100 x the largest deviation between the model in
float64 and in np.longdouble (the model's own rounding), at least 4 ulp of the quantity's largest magnitude, and for the
samples never above the project's 1e-8 of the peak.  The contour and shape models have no long-double path: their bar
is that 1e-8 of the peak.  Codes, first-knot phases, amplitudes at beta = 1, the zero pattern of the amplitudes and
everything compared between two runs of the kernels are exact.  No cell is left out (test_modify_cases_cpu.py shows
that every whole-turn count of every case is decided with 1e-9 to spare).  Every measured deviation is printed and
recorded next to its bar (conftest.record_measurement)."""
import numpy as np
import pytest

import model_contour_ref as MC
import model_shape_ref as MS
import model_synthesis_ref as M
import modify_cases as C
from conftest import record_measurement
from synth_parent_cases import split
from test_gpu_interp_stage import bar_of, by_column

pytestmark = pytest.mark.gpu

CASES = C.cases()
NAMES = [c["name"] for c in CASES]
SENTINEL = 1e300
GUARD = 64                      # sentinel samples either side of the out buffer
PEAK_BAR = 1e-8                 # the project's bound on resynthesised samples, relative to the peak
LD = np.longdouble
MAPS = ["chunks", "k300", "step2", "start"]           # the cases of the contour map and of the shape phase
SETTING_IDS = ["rho%g_beta%g_%s" % (r, b, "env" if e else "noenv") for r, b, e in C.SETTINGS]


def case(name):
    return CASES[NAMES.index(name)]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from eaqhm_amd.functions import _ctx
    return _ctx(0)


_KNOTS, _AMP, _SAMPLES = {}, {}, {}


def knots(name):
    """(code, R, ph0) of the float64 model and (R, ph0) of the long-double one, once per case."""
    if name not in _KNOTS:
        c = case(name)
        code, _, _, R, ph0 = M.knot_phases(c["records"], c["step"], c["fs"])
        _, _, _, Rl, ph0l = M.knot_phases(c["records"], c["step"], c["fs"], LD)
        _KNOTS[name] = (code, R, ph0, Rl, ph0l)
    return _KNOTS[name]


def amplitudes(name, beta, env):
    if (name, beta, env) not in _AMP:
        c = case(name)
        K = c["Kmax"]
        am, fm = c["records"][:, :K], c["records"][:, K:2 * K]
        _AMP[name, beta, env] = (M.envelope_amplitudes(am, fm, c["fs"], beta, env),
                                 M.envelope_amplitudes(am, fm, c["fs"], beta, env, LD))
    return _AMP[name, beta, env]


def samples(name, setting):
    if (name, setting) not in _SAMPLES:
        c = case(name)
        rho, beta, env = setting
        _SAMPLES[name, setting] = tuple(M.synthesize(c["records"], c["step"], c["fs"], c["L"], rho, beta, env, dtype=dt)
                                        for dt in (np.float64, LD))
    return _SAMPLES[name, setting]


class Dev:
    """Device buffers of one case and the three calls."""

    def __init__(self, ctx, c):
        import torch
        self.torch, self.ctx, self.c = torch, ctx, c
        self.n, self.K, self.D, self.fs, self.L = c["No_ti"], c["Kmax"], c["step"], c["fs"], c["L"]
        self.rec = self.dev(c["records"])
        self.code = self.full((self.n, self.K), 99, torch.uint8)
        self.mom = self.full((self.n, self.K + 1), SENTINEL)
        ctx.spline_solve(self.rec, self.n, self.K, self.D, self.code, self.mom)
        ctx.sync()
        self._prep = {}

    def dev(self, a):
        return self.torch.as_tensor(np.array(a, dtype=np.float64, order="C"), device=self.ctx.device)

    def full(self, shape, value, dtype=None):
        return self.torch.full(shape, value, dtype=dtype or self.torch.float64, device=self.ctx.device)

    def prep(self, beta, env, gain=None, key=None):
        """modify_prep into sentinel-filled amp, R, ph0 (device tensors); beta a number or one value per instant."""
        key = (float(beta), bool(env)) if key is None else key
        if key not in self._prep:
            amp, R, ph0 = (self.full((self.n, self.K), SENTINEL) for _ in range(3))
            beta_d = self.dev(np.broadcast_to(beta, (self.n,)))
            self.ctx.modify_prep(self.rec, self.code, self.mom, self.n, self.K, self.D, self.fs, beta_d,
                                 None if gain is None else self.dev(gain), None, env, amp, R, ph0)
            self.ctx.sync()
            self._prep[key] = (amp, R, ph0)
        return self._prep[key]

    def synth(self, prep, rho, beta, L_out, ranges=None, curve=None, shape=None):
        """modify_synth over `ranges` (default the whole output), each into a fresh buffer that carries GUARD sentinel
        samples either side of the output.  Nothing outside a range may be written: returns the assembled samples."""
        amp, R, ph0 = prep
        out = np.full(L_out, np.nan)
        curve_d = None if curve is None else (self.dev(curve[0]), self.dev(curve[1]), self.dev(curve[2]), float(curve[3]))
        shape_d = None if shape is None else (self.dev(shape[0]), self.dev(shape[1]))
        for lo, hi in (ranges or [(0, L_out)]):
            buf = self.full((L_out + 2 * GUARD,), SENTINEL)
            self.ctx.modify_synth(self.rec, self.code, self.mom, amp, R, ph0, self.n, self.K, self.D, self.fs, rho, beta,
                                  L_out, lo, hi, buf[GUARD:], curve_d, shape_d)
            self.ctx.sync()
            got = buf.cpu().numpy()
            assert np.all(got[:GUARD + lo] == SENTINEL) and np.all(got[GUARD + hi:] == SENTINEL), (lo, hi)
            assert not np.any(got[GUARD + lo:GUARD + hi] == SENTINEL), (lo, hi)
            out[lo:hi] = got[GUARD + lo:GUARD + hi]
        return out


_DEV = {}


def dev_of(ctx, name):
    if name not in _DEV:
        _DEV[name] = Dev(ctx, case(name))
    return _DEV[name]


def peak_of(ref, n_in):
    """The peak the 1e-8 refers to: that of the samples up to the image of the last knot.  Past it only the a0 spline
    sounds, carried on with its last cubic piece, which at step 2 grows to hundreds of times the partials 133 samples
    out; a bar taken from there would let the partials off.  The errors are taken over every sample all the same."""
    return float(np.abs(ref[:max(int(n_in), 1)]).max())


def last_knot_image(c, rho):
    return int(np.floor(rho * ((c["No_ti"] - 1) * c["step"]))) + 1


def measure(label, got, ref, ref_l, n_in):
    """Samples against the float64 model with the long-double model's bar; returns err / bar."""
    assert got.shape == ref.shape and np.all(np.isfinite(got)), label
    peak = peak_of(ref, n_in)
    bar, dev = bar_of(ref, ref_l, PEAK_BAR * peak)
    err = float(np.abs(got - ref).max())
    print("%s: model dev %.3g gpu err %.3g bar %.3g (peak %.3g)" % (label, dev, err, bar, peak))
    record_measurement("modify_direct_%s" % label, model_dev=dev, gpu_err=err, bar=bar, err_over_bar=err / bar,
                       err_over_peak=err / peak)
    return err / bar


# ------------------------------------------------------------------------------------------ prep and scan
@pytest.mark.parametrize("name", NAMES)
def test_codes_first_knot_phases_and_unwrapped_knot_phases(ctx, name):
    c = case(name)
    code_m, R_m, ph0_m, R_l, _ = knots(name)
    d = dev_of(ctx, name)
    code = d.code.cpu().numpy()
    assert np.array_equal(code, code_m), np.argwhere(code != code_m)[:5]
    worst = 0.0
    for beta, env in sorted({(b, e) for _, b, e in c["settings"]}):
        amp, R, ph0 = (t.cpu().numpy() for t in d.prep(beta, env))
        for key, a in (("amp", amp), ("R", R), ("ph0", ph0)):
            assert not np.any(a == SENTINEL), (key, beta, env)                 # every cell written
        assert np.array_equal(ph0, ph0_m), (beta, env, np.argwhere(ph0 != ph0_m)[:5])
        assert np.all(ph0[code_m <= 1] == 0) and np.all(R[code_m <= 1] == 0)
        ratio, dev, err, bar = by_column(R, R_m, R_l)
        print("%s beta %g R: worst slot: model dev %.3g gpu err %.3g bar %.3g" % (name, beta, dev, err, bar))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, beta, env, err, bar)
    record_measurement("modify_direct_R_%s" % name, err_over_bar=worst)
    # R and ph0 do not depend on beta or on the envelope: bit for bit the same from every prep
    preps = [d.prep(b, e) for _, b, e in c["settings"]]
    for amp, R, ph0 in preps[1:]:
        assert self_equal(R, preps[0][1]) and self_equal(ph0, preps[0][2])


def self_equal(a, b):
    return bool((a == b).all().item())


@pytest.mark.parametrize("name", NAMES)
def test_knot_amplitudes(ctx, name):
    c = case(name)
    K = c["Kmax"]
    am = c["records"][:, :K]
    d = dev_of(ctx, name)
    worst = 0.0
    for beta, env in sorted({(b, e) for _, b, e in c["settings"]}):
        amp = d.prep(beta, env)[0].cpu().numpy()
        A, A_l = amplitudes(name, beta, env)
        if beta == 1.0:
            assert np.array_equal(amp, am), (name, env)
            continue
        assert np.array_equal(amp != 0, A != 0), (name, beta, env)          # inactive and muted cells exactly 0
        ratio, dev, err, bar = by_column(amp, A, A_l)
        print("%s beta %g env %d amp: worst slot: model dev %.3g gpu err %.3g bar %.3g" % (name, beta, env, dev, err, bar))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, beta, env, err, bar)
        if not env:
            assert np.array_equal(amp, A)                                       # without the envelope: am or 0
    record_measurement("modify_direct_amp_%s" % name, err_over_bar=worst)


def test_harm125_node_hits_and_the_mute(ctx):
    """At beta = 2 every read lands on a node: the amplitude is that node's, through log and exp alone; the partial at
    4000 Hz is muted (2 f == fs / 2) and the one at 3875 Hz is not."""
    c = case("harm125")
    K = c["Kmax"]
    am = c["records"][:, :K]
    slot = c["slot_of"]
    amp = dev_of(ctx, "harm125").prep(2.0, True)[0].cpu().numpy()
    for i in (0, 1, 2, 4, 6, 7):
        assert amp[i, slot[31]] == 0 and amp[i, slot[30]] > 0 and np.all(amp[i, slot[32:]] == 0)
        for h in (0, 3, 8, 14):                                                 # harmonic h+1 reads harmonic 2(h+1)'s node
            assert abs(amp[i, slot[h]] / am[i, slot[2 * h + 1]] - 1.0) <= 8 * np.finfo(np.float64).eps
    assert np.all(amp[C.HARM_NONE] == 0) and np.count_nonzero(amp[C.HARM_SINGLE]) == 1


# ------------------------------------------------------------------------------------------ the scalar map
PAIRS = [(c["name"], s) for c in CASES for s in c["settings"]]                  # `long` names its own settings


@pytest.mark.parametrize("name, setting", PAIRS, ids=["%s-%s" % (n, SETTING_IDS[C.SETTINGS.index(s)]) for n, s in PAIRS])
def test_samples_whole_and_in_three_ranges(ctx, name, setting):
    c = case(name)
    rho, beta, env = setting
    d = dev_of(ctx, name)
    ref, ref_l = samples(name, setting)
    L_out = int(np.rint(rho * c["L"]))
    assert len(ref) == L_out
    prep = d.prep(beta, env)
    whole = d.synth(prep, rho, beta, L_out)
    ratio = measure("samples_%s_%s" % (name, SETTING_IDS[C.SETTINGS.index(setting)]), whole, ref, ref_l,
                    last_knot_image(c, rho))
    assert ratio <= 1.0, (name, setting, ratio)
    ranges = split(L_out, 64, c["step"]) if c["step"] > 1 else split(L_out, 64)
    for lo, hi in ranges[1:]:
        assert lo % 64 and lo % c["step"]
    parts = d.synth(prep, rho, beta, L_out, ranges)
    assert np.array_equal(parts, whole), np.flatnonzero(parts != whole)[:5]


# ------------------------------------------------------------------------------------------ contour map, shape phase
def contour_inputs(c, rho, beta):
    from eaqhm_amd.records import contour_time_map
    tm = contour_time_map(rho, beta, c["step"], c["L"])
    return tm, (tm["C"], tm["rate"], tm["gain"], tm["rate_min"])


def peak_measure(label, got, ref, n_in):
    assert got.shape == ref.shape and np.all(np.isfinite(got)), label
    peak = peak_of(ref, n_in)
    err = float(np.abs(got - ref).max())
    print("%s: gpu err %.3g, %.3g of the peak (bar %.3g)" % (label, err, err / peak, PEAK_BAR))
    record_measurement("modify_direct_%s" % label, gpu_err=err, err_over_peak=err / peak, bar_over_peak=PEAK_BAR,
                       err_over_bar=err / (PEAK_BAR * peak))
    return err / peak


@pytest.mark.parametrize("name", MAPS)
def test_contour_map(ctx, name):
    c = case(name)
    d = dev_of(ctx, name)
    rho, beta = C.contour_scales(c["No_ti"])
    tm, curve = contour_inputs(c, rho, beta)
    ref = MC.synthesize_contour(c["records"], c["step"], c["fs"], c["L"], rho, beta, True)
    assert len(ref) == tm["L_out"]
    prep = d.prep(beta, True, gain=tm["gain"], key="contour")
    whole = d.synth(prep, 0.0, 0.0, tm["L_out"], curve=curve)
    assert peak_measure("contour_%s" % name, whole, ref, int(np.floor(tm["C"][-1])) + 1) <= PEAK_BAR
    parts = d.synth(prep, 0.0, 0.0, tm["L_out"], split(tm["L_out"], 64, max(c["step"], 2)), curve=curve)
    assert np.array_equal(parts, whole)


@pytest.mark.parametrize("name", MAPS)
def test_shape_phase_on_both_maps(ctx, name):
    from eaqhm_amd.records import _records_f0, fundamental_advance
    c = case(name)
    d = dev_of(ctx, name)
    n, D, fs = c["No_ti"], c["step"], c["fs"]
    rho, beta = 1.5, 1.2
    f0 = _records_f0(c["records"], c["Kmax"])
    assert np.array_equal(f0, MS.model_f0(c["records"])) or np.allclose(f0, MS.model_f0(c["records"]), rtol=1e-14, atol=0)
    prep = d.prep(beta, True)                                                   # the shape mode's prep: Delta unweighted
    # the scalar map
    S = fundamental_advance(f0, np.full(n - 1, beta * rho), D, fs)
    L_out = int(np.rint(rho * c["L"]))
    ref = MS.synthesize_shape(c["records"], D, fs, c["L"], rho, beta, True, f0=f0)
    whole = d.synth(prep, rho, beta, L_out, shape=(f0, S))
    assert peak_measure("shape_scalar_%s" % name, whole, ref, last_knot_image(c, rho)) <= PEAK_BAR
    assert np.array_equal(d.synth(prep, rho, beta, L_out, split(L_out, 64, max(D, 2)), shape=(f0, S)), whole)
    # the contour map: the same scales as constant contours, then the contour pair of test_contour_map
    for label, rv, bv in (("const", np.full(n, rho), np.full(n, beta)), ("pair",) + C.contour_scales(n)):
        tm, curve = contour_inputs(c, rv, bv)
        S = fundamental_advance(f0, tm["gain"], D, fs)
        ref = MS.synthesize_shape(c["records"], D, fs, c["L"], rv, bv, True, f0=f0)
        assert len(ref) == tm["L_out"]
        prep_c = d.prep(bv, True, key="shape_" + label)
        whole = d.synth(prep_c, 0.0, 0.0, tm["L_out"], curve=curve, shape=(f0, S))
        assert peak_measure("shape_contour_%s_%s" % (label, name), whole, ref,
                            int(np.floor(tm["C"][-1])) + 1) <= PEAK_BAR
        parts = d.synth(prep_c, 0.0, 0.0, tm["L_out"], split(tm["L_out"], 64, max(D, 2)), curve=curve, shape=(f0, S))
        assert np.array_equal(parts, whole)


# ------------------------------------------------------------------------------------------ the public API
def test_public_api_on_the_start_runs(ctx):
    """eaQHMSynthesis on the arrays form of `start`: the three runs whose pad instants are their own knots synthesised
    NaN before DESIGN.md §9 defined their nodes."""
    import eaqhm_amd
    c = case("start")
    n, K, D = c["No_ti"], c["Kmax"], c["step"]
    rec = c["records"]
    det = dict(ti=np.arange(n) * D, isVoiced=np.ones(n, bool), a0=rec[:, 3 * K].copy(), amplitudes=rec[:, :K].copy(),
               frange=rec[:, K:2 * K].copy(), pk=rec[:, 2 * K:3 * K].copy())
    assert np.array_equal(eaqhm_amd.unpack_model(det)["records"], rec)
    for setting, sid in zip(C.SETTINGS, SETTING_IDS):
        rho, beta, env = setting
        out = eaqhm_amd.eaQHMSynthesis(det, c["fs"], c["L"], time_scale=rho, pitch_scale=beta, preserve_envelope=env)
        ref, ref_l = samples("start", setting)
        assert measure("api_start_%s" % sid, out, ref, ref_l, last_knot_image(c, rho)) <= 1.0, setting
        # the first intervals, where the three runs lie, hold sound
        assert np.abs(out[:int(rho * 2 * D)]).max() > 0


def test_falling_harmonic_count_from_the_first_instant(ctx):
    """model_from_parameters on f0 = 120 Hz rising from the first instant at 16 kHz: the top harmonic is under fs/2 for
    the first three instants only, a 3-run at 0-2."""
    import eaqhm_amd
    n, fs, step = 40, 16000, 80
    f0 = 120.0 + 0.5 * np.arange(n)
    ceps = np.zeros((n, 9))
    ceps[:, 0] = np.log(0.05)
    ceps[:, 1] = 0.4 + 0.1 * np.sin(np.arange(n) / 5.0)
    ceps[:, 3] = -0.2
    det = eaqhm_amd.model_from_parameters(f0, ceps, fs, step)
    m = eaqhm_amd.unpack_model(det)
    rec = m["records"]
    K = m["Kmax"]
    _, runs = M.run_codes(rec[:, :K] != 0)
    firsts = [r[0] for r in runs if r]
    assert (0, 2) in firsts                                                    # a run that divided by zero
    L = (n - 1) * step + 1 + 133
    for rho, beta in ((1.0, 1.0), (1.5, 1.2)):
        out = eaqhm_amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta)
        ref = M.synthesize(rec, step, fs, L, rho, beta)
        ref_l = M.synthesize(rec, step, fs, L, rho, beta, dtype=LD)
        assert measure("api_falling_count_rho%g_beta%g" % (rho, beta), out, ref, ref_l,
                       int(np.floor(rho * (n - 1) * step)) + 1) <= 1.0
        env = eaqhm_amd.eaQHMSynthesis(det, fs, L, time_scale=rho, pitch_scale=beta, envelope=ceps)
        assert np.all(np.isfinite(env))
