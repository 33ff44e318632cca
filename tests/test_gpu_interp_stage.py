"""The kernels of csrc/eaqhm_interp.hip (eaqhm_spline_kernel, eaqhm_spline_edge_kernel, eaqhm_eval_kernel,
eaqhm_srer_kernel, eaqhm_phase_integrate_kernel) through hip.Context, cell by cell against the NumPy model of the stage
(tests/interp_stage_ref.py) on its generated cases: every run shape, the three block sizes of the evaluation, step
below and above the block, tight and long signals.

Bars.  Per case, quantity and column (slot; the a0 spline is a column of its own) 100 x the largest deviation between the model in float64 and in np.longdouble (the model's
own rounding), at least 4 ulp of the quantity's largest magnitude, never above the project's TOL_AM_REL / TOL_FM_HZ /
TOL_PH_RAD and the 1e-9 on s_hat.  A cell is left out only where the model itself decides with less than 1e-9 to spare
(at most 0.1 % per case; tests/test_interp_stage_cpu.py shows the model leaves out none, so any is printed).  Integer
outputs (codes, limbs) and everything compared between two runs of the kernels are exact.  Every measured deviation is
printed and recorded next to its bar (conftest.record_measurement)."""
import numpy as np
import pytest

import interp_stage_ref as R
from conftest import record_measurement
from test_gpu_parity import TOL_AM_REL, TOL_FM_HZ, TOL_PH_RAD, TOL_SRER_DB

pytestmark = pytest.mark.gpu

CASES = R.cases()
NAMES = [c["name"] for c in CASES]
BIG = [c["name"] for c in CASES if c["No_ti"] > 6]
SENTINEL = 1e300
EPS = np.finfo(np.float64).eps
MARGIN = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from eaqhm_amd.functions import _ctx
    return _ctx(0)


_MODEL = {}


def model(name):
    """(case, float64 model, longdouble model) — computed once per case."""
    if name not in _MODEL:
        c = CASES[NAMES.index(name)]
        _MODEL[name] = (c, R.interpolate(c["records"], c["step"], c["fs"], c["L"], c["target"]),
                        R.interpolate(c["records"], c["step"], c["fs"], c["L"], c["target"], dtype=np.longdouble))
    return _MODEL[name]


def bar_of(ref, ref_l, cap=None):
    """(bar, model deviation): 100 x |float64 - longdouble|, at least 4 ulp of the magnitude, at most `cap`."""
    dev = float(np.abs(ref - ref_l).max(initial=0.0))
    bar = max(100.0 * dev, 4.0 * EPS * float(np.abs(ref).max(initial=0.0)))
    return (bar if cap is None else min(bar, cap)), dev


def by_column(got, ref, ref_l, keep=None, cap=None):
    """The same rule per column of a 2-D table, so that a quiet slot is judged by its own size.  Returns (worst
    err / bar, the model deviation, error and bar of that column); cells where keep is False are left out."""
    worst = (0.0, 0.0, 0.0, 0.0)
    for k in range(ref.shape[1]):
        m = slice(None) if keep is None else keep[:, k]
        bar, dev = bar_of(ref[m, k], ref_l[m, k], cap)
        err = float(np.abs(got[m, k] - ref[m, k]).max(initial=0.0))
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else np.inf)
        if ratio >= worst[0]:
            worst = (ratio, dev, err, bar)
    return worst


class Stage:
    """Device buffers of one case and the two calls."""

    def __init__(self, ctx, case, records=None, target=None):
        import torch
        self.torch, self.ctx, self.case = torch, ctx, case
        self.T, self.K, self.D, self.L, self.fs = case["No_ti"], case["Kmax"], case["step"], case["L"], case["fs"]
        self.rec = self.dev(case["records"] if records is None else records)
        tg = case["target"] if target is None else target
        self.target = self.dev(tg)
        with np.errstate(invalid="ignore"):
            self.std_det = float(np.std(tg))
        self.code, self.mom = self.solve()

    def dev(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a), device=self.ctx.device)

    def full(self, shape, value, dtype=None):
        return self.torch.full(shape, value, dtype=dtype or self.torch.float64, device=self.ctx.device)

    def solve(self, i_lo=0, i_hi=None):
        code = self.full((self.T, self.K), 99, self.torch.uint8)
        mom = self.full((self.T, self.K + 1), SENTINEL)
        self.ctx.spline_solve(self.rec, self.T, self.K, self.D, code, mom, i_lo, i_hi)
        self.ctx.sync()
        return code, mom

    def evaluate(self, t_lo=0, t_hi=None, s_lo=None, s_hi=None, pad=(0, 0), synth=True, tracks=True):
        """One eaqhm_eval_synth into sentinel-filled buffers.  The track window starts pad[0] samples before t_lo (as
        far as the signal goes) and ends pad[1] after t_hi.  Returns numpy: am, fm (K, track_len), track_t0, ph_knot,
        s_hat, sums (16 doubles), limbs (8 Python ints)."""
        t_hi = self.L if t_hi is None else t_hi
        s_lo = t_lo if s_lo is None else s_lo
        s_hi = t_hi if s_hi is None else s_hi
        t0 = max(0, t_lo - pad[0])
        w = t_hi + pad[1] - t0
        am = fm = ph_knot = s_hat = partials = sums = None
        if tracks:
            am, fm = self.full((self.K, w), SENTINEL), self.full((self.K, w), SENTINEL)
        if synth:
            ph_knot, s_hat = self.full((self.T, self.K), SENTINEL), self.full((self.L,), SENTINEL)
            partials = self.full((self.ctx.eval_partials_len(t_lo, t_hi, self.D),), 0.0)
            sums = self.full((16,), SENTINEL)
        self.ctx.eval_synth(self.rec, self.code, self.mom, self.T, self.K, self.D, self.fs, self.L, t_lo, t_hi, s_lo, s_hi,
                            self.target if synth else None, self.std_det, am, fm, t0 if tracks else 0, w if tracks else 0,
                            ph_knot, s_hat, partials, sums)
        self.ctx.sync()
        out = dict(t0=t0)
        for name, buf in (("am", am), ("fm", fm), ("ph_knot", ph_knot), ("s_hat", s_hat), ("sums", sums)):
            out[name] = None if buf is None else buf.cpu().numpy()
        if synth:
            out["limbs"] = [int(v) for v in sums.view(self.torch.int64)[8:16].cpu().numpy()]
        return out


_STAGE = {}


def stage(ctx, name):
    if name not in _STAGE:
        _STAGE[name] = Stage(ctx, CASES[NAMES.index(name)])
    return _STAGE[name]


def cuts_of(L, D, fractions):
    """Piece boundaries inside (0, L) that are multiples of neither 16 nor the step."""
    out = []
    for f in fractions:
        c = max(1, int(f * L))
        while c % 16 == 0 or (D > 1 and c % D == 0) or c in out:
            c += 1
        if c < L:
            out.append(c)
    return [0] + sorted(out) + [L]


# ------------------------------------------------------------------------------------------ spline_solve
@pytest.mark.parametrize("name", NAMES)
def test_codes_and_moments(ctx, name):
    case, ref, ref_l = model(name)
    st = stage(ctx, name)
    code, mom = st.code.cpu().numpy(), st.mom.cpu().numpy()
    assert np.array_equal(code, ref["code"]), np.argwhere(code != ref["code"])[:5]
    ratio, dev, err, bar = by_column(mom, ref["mom"], ref_l["mom"])
    print("%s mom: worst column: model dev %.3g gpu err %.3g bar %.3g" % (name, dev, err, bar))
    record_measurement("interp_stage_moments_%s" % name, model_dev=dev, gpu_err=err, bar=bar, err_over_bar=ratio)
    assert ratio <= 1.0, (name, err, bar)
    assert np.all(mom[:, :case["Kmax"]][code != 2] == 0)


@pytest.mark.parametrize("name", BIG)
def test_subrange_solve(ctx, name):
    case, ref, ref_l = model(name)
    st = stage(ctx, name)
    T, K = st.T, st.K
    code_f, mom_f = st.code.cpu().numpy(), st.mom.cpu().numpy()
    runs = R.runs_of(case["records"][:, 5 % K] != 0) + R.runs_of(case["records"][:, K - 1] != 0)
    long_run = max(runs, key=lambda ab: ab[1] - ab[0])
    mid = (long_run[0] + long_run[1]) // 2                      # an edge inside a run
    wins = [(1, T), (2, T // 2), (3, T // 3 + 1), (4, T - 3), (5, min(47, T)), (mid, min(mid + 40, T)),
            (max(long_run[0] - 7, 0), mid), (T - 9, T)]
    for lo, hi in wins:
        assert 0 <= lo < hi <= T
        code, mom = st.solve(lo, hi)
        code, mom = code.cpu().numpy(), mom.cpu().numpy()
        assert np.array_equal(code[lo:hi], ref["code"][lo:hi]) and np.array_equal(code[:4], ref["code"][:4]), (lo, hi)
        assert np.array_equal(mom[lo:hi], mom_f[lo:hi]), (lo, hi)          # the full solve, bit for bit
        assert by_column(mom[lo:hi], ref["mom"][lo:hi], ref_l["mom"][lo:hi])[0] <= 1.0, (lo, hi)
        # nothing written beyond the two instants either side the end conditions need, and rows 0..3
        out = np.ones(T, bool)
        out[max(lo - 2, 0):min(hi + 2, T)] = False
        out[:4] = False
        assert np.all(code[out] == 99) and np.all(mom[out] == SENTINEL), (lo, hi)


# ------------------------------------------------------------------------------------------ eval_synth
@pytest.mark.parametrize("name", NAMES)
def test_every_cell(ctx, name):
    case, ref, ref_l = model(name)
    st = stage(ctx, name)
    got = st.evaluate()
    K, L = st.K, st.L
    for key in ("am", "fm", "ph_knot", "s_hat"):
        assert not np.any(got[key] == SENTINEL), key                      # every cell written, empty slots included
    assert np.all(got["am"][0] == 0) and np.all(got["fm"][0] == 0) and np.all(got["ph_knot"][:, 0] == 0)
    bad = R.excluded_cells(ref, st.D, MARGIN)
    n_bad = int(bad.sum())
    assert n_bad <= 1e-3 * bad.size
    if n_bad:
        print("%s: %d cells under the model's own decision margin left out" % (name, n_bad))
    keep = ~bad
    bad_t = bad.any(axis=1)
    bad_i = bad[np.arange(st.T) * st.D]
    rows = {}
    for key, g, r, rl, cap, kp in (
            ("am", got["am"].T, ref["am"], ref_l["am"], "rel", keep),
            ("fm", got["fm"].T, ref["fm_next"], ref_l["fm_next"], TOL_FM_HZ, keep),
            ("ph_knot", got["ph_knot"], ref["ph_knot"], ref_l["ph_knot"], TOL_PH_RAD, ~bad_i),
            ("s_hat", got["s_hat"], ref["s_hat"], ref_l["s_hat"], 1e-9, ~bad_t)):
        if r.ndim == 1:
            bar, dev = bar_of(r[kp], rl[kp], cap)
            err = float(np.abs(g[kp] - r[kp]).max(initial=0.0))
        elif cap == "rel":      # the project's amplitude bound is relative: here to the slot's own largest amplitude
            worst = [by_column(g[:, k:k + 1], r[:, k:k + 1], rl[:, k:k + 1], kp[:, k:k + 1],
                               TOL_AM_REL * float(np.abs(r[:, k]).max())) for k in range(r.shape[1])]
            _, dev, err, bar = max(worst)
        else:
            _, dev, err, bar = by_column(g, r, rl, kp, cap)
        rows[key] = (dev, err, bar)
        print("%s %s: worst column: model dev %.3g gpu err %.3g bar %.3g" % (name, key, dev, err, bar))
    record_measurement("interp_stage_cells_%s" % name, excluded=n_bad, cells=int(bad.size),
                       block=R.eval_block_samples(K, st.D)[0],
                       **{"%s_%s" % (k, f): v for k, row in rows.items() for f, v in zip(("model_dev", "gpu_err", "bar"), row)})
    for key, (dev, err, bar) in rows.items():
        assert err <= bar, (name, key, err, bar)
    # the zero pattern is part of the result: the next adaptation reads fm == 0 as "slot not active here"
    assert np.array_equal(got["fm"].T[keep] != 0, ref["fm_next"][keep] != 0)
    assert np.array_equal(got["am"].T != 0, ref["am"] != 0)


@pytest.mark.parametrize("name", NAMES)
def test_ranges_track_window_and_limbs(ctx, name):
    case, _, _ = model(name)
    st = stage(ctx, name)
    L, D = st.L, st.D
    whole = st.evaluate()
    shift = R.error_sum_shift(st.std_det)
    assert whole["limbs"][7] == shift
    for fractions in ((0.37,), (0.23, 0.52, 0.81)):
        cuts = cuts_of(L, D, fractions)
        assert 3 <= len(cuts) <= 5
        total = [0] * 8
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = st.evaluate(lo, hi, pad=(5, 7))
            t0 = part["t0"]
            assert lo == 0 or t0 > 0
            for key in ("am", "fm"):
                assert np.array_equal(part[key][:, lo - t0:hi - t0], whole[key][:, lo:hi]), (key, lo, hi)
                assert np.all(part[key][:, :lo - t0] == SENTINEL) and np.all(part[key][:, hi - t0:] == SENTINEL)
            assert np.array_equal(part["s_hat"][lo:hi], whole["s_hat"][lo:hi])
            assert np.all(part["s_hat"][:lo] == SENTINEL) and np.all(part["s_hat"][hi:] == SENTINEL)
            inst = np.arange(st.T) * D
            inside = (inst >= lo) & (inst < hi)
            assert np.array_equal(part["ph_knot"][inside], whole["ph_knot"][inside])
            assert np.all(part["ph_knot"][~inside] == SENTINEL)
            assert part["limbs"][7] == shift
            total = [a + b for a, b in zip(total, part["limbs"][:7] + [0])]
        # the words add up as integers; what they stand for — the two sums and the count — is what must agree
        assert R.ints_of(total)[:3] == R.ints_of(whole["limbs"])[:3], (cuts, total, whole["limbs"])
    # error sums over a strict sub-range of the evaluated range = the sub-range evaluated alone
    cuts = cuts_of(L, D, (0.23, 0.81))
    lo, hi = (cuts[1], cuts[2]) if len(cuts) == 4 and cuts[2] - cuts[1] > 10 else (0, L)
    s_lo, s_hi = lo + 3, hi - 5
    if s_hi > s_lo:
        assert R.ints_of(st.evaluate(lo, hi, s_lo, s_hi)["limbs"]) == R.ints_of(st.evaluate(s_lo, s_hi)["limbs"])


@pytest.mark.parametrize("name", NAMES)
def test_track_only_pass(ctx, name):
    st = stage(ctx, name)
    whole = st.evaluate()
    only = st.evaluate(synth=False)
    assert np.array_equal(only["am"], whole["am"]) and np.array_equal(only["fm"], whole["fm"])
    cuts = cuts_of(st.L, st.D, (0.41,))
    part = st.evaluate(cuts[1], st.L, pad=(3, 0), synth=False)
    t0 = part["t0"]
    assert np.array_equal(part["am"][:, cuts[1] - t0:], whole["am"][:, cuts[1]:])
    assert np.array_equal(part["fm"][:, cuts[1] - t0:], whole["fm"][:, cuts[1]:])
    assert np.all(part["fm"][:, :cuts[1] - t0] == SENTINEL)


def check_sums(st, got, target, n):
    """sums_out against the header's contract recomputed in Python integers from the returned s_hat."""
    from eaqhm_amd.engine import srer_from_limbs
    d = target - got["s_hat"]
    tot, tot2, bad, sh = R.fixed_point_sums(d, st.std_det)
    assert R.ints_of(got["limbs"]) == (tot, tot2, bad, sh)
    s = got["sums"]
    assert s[2] == n
    if bad:
        assert np.isnan(s[3]) and np.isnan(srer_from_limbs(got["limbs"], n, st.std_det))
        return None
    a, b = np.ldexp(tot / (1 << 60), -sh), np.ldexp(tot2 / (1 << 64), -2 * sh)
    assert abs(s[0] - a) <= 8 * EPS * abs(a) and abs(s[1] - b) <= 8 * EPS * abs(b)
    srer = srer_from_limbs(got["limbs"], n, st.std_det)
    assert abs(s[3] - srer) <= 1e-9
    return float(srer)


@pytest.mark.parametrize("name", NAMES)
def test_error_sums_exact(ctx, name):
    case, ref, _ = model(name)
    st = stage(ctx, name)
    got = st.evaluate()
    srer = check_sums(st, got, case["target"], st.L)
    print("%s SRER: kernel %.9f model %.9f" % (name, srer, float(ref["srer"])))
    record_measurement("interp_stage_srer_%s" % name, gpu=srer, model=float(ref["srer"]))
    assert abs(srer - float(ref["srer"])) <= TOL_SRER_DB


def test_error_sums_count_what_cannot_be_summed(ctx):
    case, _, _ = model(NAMES[0])
    tg = case["target"].copy()
    tg[[11, 1234, 4000]] = [np.nan, np.inf, 2.0 ** 20 + 1.0]
    st = Stage(ctx, case, target=tg)
    st.std_det = float(np.std(case["target"]))                 # the level of the signal proper
    got = st.evaluate()
    assert got["limbs"][6] == 3
    assert check_sums(st, got, tg, st.L) is None


def test_a_click_far_above_the_level_is_summed(ctx):
    """One sample 2^19 times the signal's standard deviation (a click in a near-silent file) still enters the sums: the
    SRER is finite and the model's.  The contract counts a sample out only from 2^20 times the level on."""
    from eaqhm_amd.engine import srer_from_limbs
    case, ref, _ = model(NAMES[0])
    K = case["Kmax"]
    rec = case["records"].copy()
    rec[:, :K] = np.ldexp(rec[:, :K], -20)
    rec[:, 3 * K] = np.ldexp(rec[:, 3 * K], -20)
    tg = np.ldexp(case["target"], -20)
    sd = float(np.std(tg))
    tg[777] = 2.0 ** 19 * sd
    want = R.interpolate(rec, case["step"], case["fs"], case["L"], tg, std_det=sd)
    st = Stage(ctx, case, records=rec, target=tg)
    st.std_det = sd                                             # the level without the click
    got = st.evaluate()
    assert got["limbs"][6] == 0
    srer = check_sums(st, got, tg, st.L)
    print("click: kernel %.9f model %.9f" % (srer, float(want["srer"])))
    record_measurement("interp_stage_srer_click", gpu=srer, model=float(want["srer"]))
    assert np.isfinite(srer) and abs(srer - float(want["srer"])) <= TOL_SRER_DB


def test_srer_across_signal_level(ctx):
    """Everything scaled by 2^-k (exact in FP64): the SRER is the same number at every level.  And a reconstruction
    that is nearly exact: the target is the model's s_hat plus noise at 1e-9 of its level.

    The contract before this one (truncation toward zero at a fixed 2^-60 / 2^-64), emulated in Python integers on
    the model's errors of this case, is 4e-8 dB off at k = 20, 0.045 dB off at k = 30, nan at k = 40, and 0.039 dB off on
    the near-exact reconstruction: the last three are what this test is for."""
    from eaqhm_amd.engine import srer_from_limbs
    name = NAMES[0]
    case, ref, ref_l = model(name)
    K = case["Kmax"]
    rows = {}
    for k in (0, 10, 20, 30, 40):
        rec = case["records"].copy()
        rec[:, :K] = np.ldexp(rec[:, :K], -k)
        rec[:, 3 * K] = np.ldexp(rec[:, 3 * K], -k)
        tg = np.ldexp(case["target"], -k)
        want = float(R.interpolate(rec, case["step"], case["fs"], case["L"], tg)["srer"])
        assert abs(want - float(ref["srer"])) <= 1e-9
        st = Stage(ctx, case, records=rec, target=tg)
        got = st.evaluate()
        srer = float(srer_from_limbs(got["limbs"], st.L, st.std_det))
        rows["k%d" % k] = abs(srer - want)
        print("level 2^-%d: kernel %.9f model %.9f" % (k, srer, want))
        assert check_sums(st, got, tg, st.L) == srer
    noise = 1e-9 * float(np.std(ref["s_hat"])) * np.random.default_rng(2).standard_normal(case["L"])
    tg = ref["s_hat"] + noise
    want = float(R.interpolate(case["records"], case["step"], case["fs"], case["L"], tg)["srer"])
    want_l = float(R.interpolate(case["records"], case["step"], case["fs"], case["L"], tg, dtype=np.longdouble)["srer"])
    st = Stage(ctx, case, target=tg)
    got = st.evaluate()
    # errors this small do not land on whole numbers of the fixed point: the words show the rounding to nearest
    d = np.ldexp(tg - got["s_hat"], R.error_sum_shift(st.std_det))
    assert np.count_nonzero(np.ldexp(d * d, 64) % 1.0) > 0.9 * st.L
    near = check_sums(st, got, tg, st.L)
    assert near == float(srer_from_limbs(got["limbs"], st.L, st.std_det))
    print("near-exact: kernel %.9f model %.9f (longdouble %.9f)" % (near, want, want_l))
    record_measurement("interp_stage_srer_levels", near_exact_gpu=near, near_exact_model=want,
                       near_exact_model_longdouble=want_l, **{"abs_err_db_%s" % k: v for k, v in rows.items()})
    for k, v in rows.items():
        assert v <= TOL_SRER_DB, (k, v)
    assert want > 150 and abs(near - want) <= TOL_SRER_DB, (near, want)


# ------------------------------------------------------------------------------------------ phase_integrate
def test_phase_integrate_knot_spacings(ctx):
    import torch
    rng = np.random.default_rng(9)
    fs = 16000.0

    def run(knots, n):
        om = 2 * np.pi / fs * (900 + 300 * np.sin(np.arange(n) / 37.0) + 20 * rng.standard_normal(n))
        ph = np.zeros(n)
        ph[knots] = -rng.uniform(-np.pi, np.pi, len(knots))
        mg = []
        ref = R.phase_integrate(om, ph, knots, margins=mg)
        ref_l = R.phase_integrate(om, ph, knots, np.longdouble)
        assert min(mg) >= 1e-6
        kn = torch.as_tensor(np.asarray(knots, dtype=np.int32), device=ctx.device)
        out = torch.full((int(knots[-1] - knots[0]) + 1,), SENTINEL, dtype=torch.float64, device=ctx.device)
        ctx.phase_integrate(torch.as_tensor(om, device=ctx.device), torch.as_tensor(ph, device=ctx.device), kn,
                            len(knots), int(knots[0]), int(knots[-1]), out)
        ctx.sync()
        return out.cpu().numpy(), ref, ref_l

    many = np.cumsum(np.concatenate(([7], rng.integers(1, 6, 1199))))
    for label, knots, n in (("spacing1", np.arange(0, 300), 300), ("one2000", np.array([0, 2000]), 2001),
                            ("knots1200", many, int(many[-1]) + 5), ("first_gt0", np.array([41, 50, 51, 77, 140]), 150)):
        got, ref, ref_l = run(knots, n)
        bar, dev = bar_of(ref, ref_l, TOL_PH_RAD)
        err = float(np.abs(got - ref).max())
        print("phase_integrate %s: model dev %.3g gpu err %.3g bar %.3g" % (label, dev, err, bar))
        record_measurement("interp_stage_phase_integrate_%s" % label, model_dev=dev, gpu_err=err, bar=bar)
        assert got.shape == ref.shape and err <= bar, (label, err, bar)


# ------------------------------------------------------------------------------------------ refusals
def test_argument_checks(ctx):
    """Host-side refusals (EAQHM_EINVAL and its message); no kernel runs with these arguments."""
    import torch
    case, _, _ = model("b64_n6_past")
    st = stage(ctx, "b64_n6_past")
    T, K, D, L, fs = st.T, st.K, st.D, st.L, st.fs

    def z(*shape, dtype=torch.float64):
        return torch.zeros(shape, dtype=dtype, device=ctx.device)

    am, fm, phk, sh, part, sums = z(K, L), z(K, L), z(T, K), z(L), z(ctx.eval_partials_len(0, L, D)), z(16)

    def ev(No_ti=T, Kmax=K, L_=L, t=(0, L), s=(0, L), win=(0, L), rec=st.rec, code=st.code, mom=st.mom):
        ctx.eval_synth(rec, code, mom, No_ti, Kmax, D, fs, L_, t[0], t[1], s[0], s[1], st.target, st.std_det, am, fm,
                       win[0], win[1], phk, sh, part, sums)

    ev()                                                                    # the good call
    ctx.sync()
    with pytest.raises(RuntimeError, match="error -1.*at least 4 analysis instants"):
        ctx.spline_solve(st.rec, 3, K, D, st.code, st.mom)
    with pytest.raises(RuntimeError, match="error -1.*bad argument"):
        ev(No_ti=3)
    with pytest.raises(RuntimeError, match="error -1.*instants beyond the signal"):
        ev(L_=(T - 1) * D, t=(0, (T - 1) * D), s=(0, (T - 1) * D), win=(0, (T - 1) * D))
    for win in ((1, L), (0, L - 1)):
        with pytest.raises(RuntimeError, match="error -1.*outside the track window"):
            ev(win=win)
    with pytest.raises(RuntimeError, match="error -1.*error range"):
        ev(t=(4, L), s=(3, L), win=(4, L - 4))
    with pytest.raises(RuntimeError, match="error -1.*error range"):
        ev(t=(0, L - 2), s=(0, L - 1))
    big = 400                                                               # 16-sample tables beyond 160 KiB of LDS
    assert R.eval_block_samples(big, D)[1] > 160 * 1024
    amb, phb = z(big, L), z(T, big)
    with pytest.raises(RuntimeError, match="error -1.*Kmax too large"):
        ctx.eval_synth(z(T, 3 * big + 1), z(T, big, dtype=torch.uint8), z(T, big + 1), T, big, D, fs, L, 0, L, 0, L,
                       st.target, st.std_det, amb, z(big, L), 0, L, phb, sh, part, sums)
    ctx.sync()
    assert ctx.abi_version == 6
