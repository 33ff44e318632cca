"""The NumPy model of the interpolation stage (tests/interp_stage_ref.py) against the oracle and SciPy, the invariants of
its case generator, and the host's decoding of the fixed-point error sums.  No GPU: tests/test_gpu_interp_stage.py
compares the kernels of csrc/eaqhm_interp.hip with this model on the same cases."""
import numpy as np
import pytest
from scipy.interpolate import make_interp_spline

import eaqhm_oracle as O
import interp_stage_ref as R

CASES = R.cases()
NAMES = [c["name"] for c in CASES]
MARGIN = 1e-9            # the exclusion margin of the GPU tests
WIDE = 1e-6              # what the generator keeps: a thousand times that


@pytest.fixture(scope="module")
def refs():
    return {c["name"]: R.interpolate(c["records"], c["step"], c["fs"], c["L"], c["target"]) for c in CASES}


def oracle_stage(case):
    """interpolate_tracks + the synthesis and SRER of Analysis.post_stage on dense (L, Kmax) arrays."""
    rec, K, L, D = R.clean_records(case), case["Kmax"], case["L"], case["step"]
    ti = np.arange(case["No_ti"]) * D + 1
    c = ti - 1
    am, fm, ph = np.zeros((L, K)), np.zeros((L, K)), np.zeros((L, K))
    am[c], fm[c], ph[c] = rec[:, :K], rec[:, K:2 * K], rec[:, 2 * K:3 * K]
    a0, fm_next = O.interpolate_tracks(rec[:, 3 * K].copy(), am, fm, ph, ti, D, case["fs"], L)
    s_hat = a0 + 2 * (am * np.cos(ph)).sum(axis=1)
    srer = 20 * np.log10(np.std(case["target"]) / np.std(case["target"] - s_hat))
    return dict(am=am, fm_recon=fm, ph=ph, fm_next=fm_next, a0=a0, s_hat=s_hat, srer=srer)


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_oracle(refs, name):
    """Same decisions, same values: the amplitudes bit for bit (one formula), the rest to the rounding of two spline
    solvers (SciPy's banded B-spline solve against the tridiagonal sweep) carried through the phase integration."""
    case = CASES[NAMES.index(name)]
    r, o = refs[name], oracle_stage(case)
    assert np.array_equal(r["am"], o["am"])
    assert np.array_equal(r["fm_next"] != 0, o["fm_next"] != 0) and np.array_equal(r["ph"] != 0, o["ph"] != 0)
    top = max(np.abs(o["fm_recon"]).max(), 1.0)
    assert np.abs(r["fm_recon"] - o["fm_recon"]).max() <= 1e-11 * top
    assert np.abs(r["ph"] - o["ph"]).max() <= 1e-9            # same branch of every round(): no 2 pi apart anywhere
    assert np.abs(r["fm_next"] - o["fm_next"]).max() <= 1e-6  # Hz; a turned unwrap would show as fs
    assert np.abs(r["a0"] - o["a0"]).max() <= 1e-12
    assert np.abs(r["s_hat"] - o["s_hat"]).max() <= 1e-9 * max(np.abs(o["s_hat"]).max(), 1.0)
    assert abs(float(r["srer"]) - o["srer"]) <= 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_moments_equal_scipy(refs, name):
    case = CASES[NAMES.index(name)]
    rec, K, D = case["records"], case["Kmax"], case["step"]
    r = refs[name]
    x = np.arange(case["No_ti"]) * float(D)
    cols = [(K, 0, case["No_ti"] - 1)]
    for k in range(K):
        cols += [(k, a, b) for a, b in R.runs_of(rec[:, k] != 0) if b - a + 1 >= 4]
    assert len(cols) > (1 if case["No_ti"] > 6 else 0)
    for k, a, b in cols:
        y = rec[a:b + 1, 3 * K] if k == K else rec[a:b + 1, K + k]
        want = make_interp_spline(x[a:b + 1], y, k=3).derivative(2)(x[a:b + 1])
        got = r["mom"][a:b + 1, k]
        # a moment is a sum of second differences of y over h^2 / 6 with weights that add up to less than 2: both
        # solvers carry the rounding of y into it, about eps max|y| 6 / h^2 per term
        bar = 1e-10 * np.abs(want).max() + 50 * np.finfo(float).eps * np.abs(y).max() * 6 / D ** 2
        assert np.abs(got - want).max() <= bar, (k, a, b)
    # nothing but runs of >= 4 carries a moment, and the codes say which cells those are
    assert np.array_equal(r["mom"][:, :K] != 0, (r["code"] == 2) & (r["mom"][:, :K] != 0))
    m = (r["code"] >= 16)
    assert np.all((((r["code"][m] - 16) >> 2) >= 2) & (((r["code"][m] - 16) >> 2) <= 3))


def test_generator_covers_run_shapes_and_geometries():
    blocks, steps, rates, lengths = set(), set(), set(), set()
    for c in CASES:
        K, D, T, L = c["Kmax"], c["step"], c["No_ti"], c["L"]
        acc = c["records"][:, :K] != 0
        assert not acc[:2].any() and not acc[T - 1:].any()                     # the reference's domain
        tbs, lds = R.eval_block_samples(K, D)
        assert c["name"].startswith("b%d_" % tbs) and lds <= 160 * 1024, (c["name"], tbs)
        blocks.add(tbs)
        steps.add(D)
        rates.add(c["fs"])
        lengths |= set(R.run_lengths(acc))
        assert L >= (T - 1) * D + 2 and (("_past" in c["name"]) == (L >= (T - 1) * D + 2 + D))
        if T > 6:
            assert not acc[:, 0].any() and acc[2:T - 1, 1].all()               # an empty slot and a full one
            assert acc[2:4, 2].all() and not acc[2:4, 3].any()                 # short runs behind accepted / empty 2..3
            assert {2, 3} <= set(R.run_lengths(acc[:, 2:3])) and {2, 3} <= set(R.run_lengths(acc[:, 3:4]))
            assert acc[T - 2, 3] and acc[2, 4]                                 # a run ends at No_ti-2, one starts at 2
            runs4 = R.runs_of(acc[:, 4])
            assert any(b[0] - a[1] == 2 for a, b in zip(runs4[:-1], runs4[1:]))  # one rejected instant apart
            amp = c["records"][:, :K][acc]
            assert amp.max() / amp.min() >= 1e6                                # six decades
            assert c["records"][:, K + 1][acc[:, 1]].max() >= c["fs"] / 2 - 201   # up to 200 Hz under Nyquist
            assert c["records"][:, K:2 * K].max() <= c["fs"] / 2 - 200
        ph = c["records"][:, 2 * K:3 * K]
        assert ph.min() > -np.pi and ph.max() <= np.pi
    assert blocks == {64, 32, 16}
    assert steps >= {1, 7, 15, 80, 240} and rates == {16000, 48000}
    assert set(R.RUN_LENGTHS) <= lengths and max(lengths) >= 200
    assert {c["No_ti"] for c in CASES} >= {4, 5, 6}
    assert any(c["L"] % 16 for c in CASES) and sum(c["L"] % 16 != 0 for c in CASES) >= 5
    assert any(c["dirty"] for c in CASES)
    dirty = [c for c in CASES if c["dirty"]][0]
    off = dirty["records"][:, :dirty["Kmax"]] == 0
    assert np.all(dirty["records"][:, dirty["Kmax"]:2 * dirty["Kmax"]][off] != 0)


@pytest.mark.parametrize("name", NAMES)
def test_no_cell_under_the_exclusion_margin(refs, name):
    case = CASES[NAMES.index(name)]
    r = refs[name]
    assert min(r["margin_round"].min(), r["margin_unwrap"].min()) >= WIDE
    assert not R.excluded_cells(r, case["step"], MARGIN).any()
    rl = R.interpolate(case["records"], case["step"], case["fs"], case["L"], case["target"], dtype=np.longdouble)
    assert not R.excluded_cells(rl, case["step"], MARGIN).any()
    assert np.array_equal(r["code"], rl["code"])
    assert np.abs(r["ph"] - rl["ph"]).max() <= 1e-9           # both arithmetics took every decision alike


def test_phase_integrate_equals_oracle():
    rng = np.random.default_rng(5)
    om = 2 * np.pi / 16000 * (300 + 50 * rng.standard_normal(400))
    kn = np.array([5, 20, 33, 64, 65, 120, 199, 399])
    ph = np.zeros(400)
    ph[kn] = rng.uniform(-np.pi, np.pi, len(kn))
    assert np.array_equal(R.phase_integrate(om, ph, kn), O.phase_integr_interpolation(om, ph, kn))
    ld = R.phase_integrate(om, ph, kn, np.longdouble)
    assert ld.dtype == np.longdouble and np.abs(ld - O.phase_integr_interpolation(om, ph, kn)).max() <= 1e-12


def test_srer_from_limbs_on_the_fixed_point_contract(refs):
    """include/eaqhm_hip.h: d' = d 2^s, s from std_det; sum rint(d' 2^60), sum rint(d'^2 2^64), a count, s.  Emulated
    here in Python integers on the model's errors, at five signal levels and for a near-exact reconstruction."""
    from eaqhm_amd.engine import error_sum_shift, srer_from_limbs
    case = CASES[0]
    r = refs[case["name"]]
    n = case["L"]
    for k in (0, 10, 20, 30, 40):
        tg = np.ldexp(case["target"], -k)
        d = tg - np.ldexp(r["s_hat"], -k)                       # exact scaling of everything
        sd = float(np.std(tg))
        assert error_sum_shift(sd) == R.error_sum_shift(sd) == error_sum_shift(float(np.std(case["target"]))) + k
        tot, tot2, bad, sh = R.fixed_point_sums(d, sd)
        assert bad == 0
        got = srer_from_limbs(R.limbs_of(tot, tot2, bad, sh), n, sd)
        assert abs(got - float(r["srer"])) <= 1e-9, (k, got, float(r["srer"]))
        parts = [R.fixed_point_sums(x, sd) for x in (d[:1000], d[1000:1001], d[1001:])]
        assert sum(p[0] for p in parts) == tot and sum(p[1] for p in parts) == tot2
    noise = 1e-9 * np.std(r["s_hat"]) * np.random.default_rng(2).standard_normal(n)
    tg = r["s_hat"] + noise
    d = tg - r["s_hat"]
    sd = float(np.std(tg))
    want = 20 * np.log10(sd / np.std(d))
    tot, tot2, bad, sh = R.fixed_point_sums(d, sd)
    got = srer_from_limbs(R.limbs_of(tot, tot2, bad, sh), n, sd)
    assert want > 170 and abs(got - want) <= 1e-7, (got, want)
    # the contract this one replaced — no shift, cut toward zero — does not meet the project's 1e-6 dB on that input
    t0, t2, bad0, sh0 = R.fixed_point_sums(d, 0.0, rounding=np.trunc)
    old = srer_from_limbs(R.limbs_of(t0, t2, bad0, sh0), n, sd)
    assert (bad0, sh0) == (0, 0) and abs(old - want) > 1e-2, (old, want)
    # a click 2^19 times the level is summed, not counted: the SRER stays finite and right
    dc = np.ldexp(case["target"], -20) - np.ldexp(r["s_hat"], -20)
    sdc = float(np.std(np.ldexp(case["target"], -20)))
    dc[77] = 2.0 ** 19 * sdc
    tot, tot2, bad, sh = R.fixed_point_sums(dc, sdc)
    assert bad == 0 and abs(srer_from_limbs(R.limbs_of(tot, tot2, bad, sh), n, sdc) - 20 * np.log10(sdc / np.std(dc))) <= 1e-9
    # non-finite and huge samples are counted, not summed
    d3 = d.copy()
    d3[[3, 30, 300]] = [np.nan, np.inf, 2.0 ** 22 * sd]  # (four times the 2^20 x level a sample may reach at most)
    tot, tot2, bad, sh = R.fixed_point_sums(d3, sd)
    assert bad == 3 and np.isnan(srer_from_limbs(R.limbs_of(tot, tot2, bad, sh), n, sd))
    assert R.ints_of(R.limbs_of(tot, tot2, bad, sh)) == (tot, tot2, bad, sh)


def test_frame_plan_keeps_the_stage_inside_its_domain():
    """FramePlan refuses analysisWindow < 3, and with 3 analyses nothing outside instants [3, No_ti-4] (functions.py:180)."""
    from types import SimpleNamespace
    from eaqhm_amd.engine import FramePlan
    fs, L, step, fstep = 16000, 16000, 15, 80
    frames = [SimpleNamespace(isVoiced=True) for _ in range(L // fstep + 2)]
    grid = np.column_stack([np.arange(len(frames)) * 0.005, np.full(len(frames), 200.0)])
    for aw in (0, 1, 2):
        with pytest.raises(ValueError, match="analysisWindow"):
            FramePlan(L, fs, grid, frames, fstep, step, 3, aw, 0)
    plan = FramePlan(L, fs, grid, frames, fstep, 240, 3, 3, 0)
    assert plan.n_frames > 0 and plan.frame_inst.min() >= 3 and plan.frame_inst.max() <= plan.No_ti - 4
