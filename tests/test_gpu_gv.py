"""The global-variance ascent on the MI355X (eaqhm_gv_ascend; convert.conversion_train(gv=) / conversion_trajectory) against
the NumPy model of DESIGN.md §12.2 (tests/gv_ref.py) in np.longdouble.  Hand-built seeded inputs only (gv_ref.CASES).

The kernel cases call eaqhm_gv_ascend directly with the float64 model's y_ML as the input Y, so that the solve's own error
stays out; Y outside the runs, `work` and the trace are NaN before the launch.  Bars, per case (u = 2^-53):
  |Y - Y_longdouble| <= 100 max(the float64 model's own difference from the long-double model, u max|Y|)
  |trace - trace_longdouble| <= 100 max(the float64 model's own difference, u x the sum of the magnitudes of the entry's
                                        two terms)
and a second launch on the same inputs gives the same bits.  tests/test_gv_cpu.py shows on the model that a result without
the global-variance term misses the first bar by more than ten times in cases A to C.

Without the term conversion_trajectory is held bit for bit to the rows of the commit before it
(tests/gv_parent_cases.py, tests/golden/gv_parent_digests.json).

End to end the rule is §12.1's (tests/test_gpu_mlpg.py): per system 100 x the model's own difference, floored at
cond_2(R) x (the solve's backward bar + the one-step bars of the posteriors and of the regression) x ||y||_2.

Measured on the MI355X (profiles/gv/parity_measurements.json): |Y - long double| 0.6 to 3.7 x the float64 model's own
difference (at most 4.2e-14), the trace at most 0.013 of its bar, end to end 4.0e-4 of the bar; the step case's variance
0.850 -> 0.9995 of gv_mean and its largest adjacent step 0.199 -> 0.213."""
import numpy as np
import pytest

import gv_ref as V
import mlpg_ref as R
from conftest import record_measurement

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


def ctx():
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    return torch, c, c.device


def dev(a, dtype=np.float64):
    torch, c, d = ctx()
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=d)


def gpu_ascend(c, with_trace=True):
    """(Y, trace) of a gv_ref case from two launches that must agree bit for bit; everything the kernels write into is NaN
    before each launch."""
    torch, k, d = ctx()
    n, dy, span, iters = c["n"], c["dy"], c["span"], c["iters"]
    out = []
    for _ in range(2):
        Y = dev(c["y_ml"])
        work = torch.full((k.gv_work_len(n, dy, span),), np.nan, dtype=torch.float64, device=d)
        trace = torch.full((iters + 1, dy), np.nan, dtype=torch.float64, device=d) if with_trace else None
        k.gv_ascend(dev(c["P"]), dev(c["r"]), n, dy, span, dev(c["start"], np.int64), dev(c["length"], np.int64),
                    len(c["start"]), dev(c["gv_mean"]), dev(c["gv_prec"]), iters, work, Y, trace)
        out.append((Y.cpu().numpy(), trace.cpu().numpy() if with_trace else None))
    assert np.array_equal(out[0][0], out[1][0], equal_nan=True)                       # the same bits on every run
    assert not with_trace or np.array_equal(out[0][1], out[1][1])
    return out[0]


def check(name, c, Y, trace):
    """Asserts both bars; records the ratios."""
    (y64, t64, _), (yld, tld, _) = c["ref64"], c["refld"]
    live = ~np.isnan(y64[:, 0])
    assert np.all(np.isnan(Y[~live])) and np.all(np.isfinite(Y[live])) and np.all(np.isfinite(trace))
    bar_y, bar_t = V.bars(c)
    err = float(np.abs(Y[live].astype(LD) - yld[live]).max())
    err_t = np.abs(trace.astype(LD) - tld).astype(np.float64)
    own = float(np.abs(y64[live].astype(LD) - yld[live]).max())
    print("gv case %s: |Y - long double| %.3g (the model's own %.3g, bar %.3g), trace / bar <= %.3g"
          % (name, err, own, bar_y, float((err_t / bar_t).max())))
    record_measurement("gv_case_%s" % name, err=err, model_diff=own, err_over_bar=err / bar_y,
                       trace_err_over_bar=float((err_t / bar_t).max()))
    assert err <= bar_y, (name, err, bar_y)
    assert np.all(err_t <= bar_t), (name, float((err_t / bar_t).max()))


# ---- the kernels
@pytest.mark.parametrize("name", ["A", "B", "C", "E", "G"])
def test_ascent_against_long_double(amd, name):
    c = V.case(name)
    Y, trace = gpu_ascend(c)
    check(name, c, Y, trace)
    if name == "E":                                                                  # rows that no run holds keep their NaN
        live = np.zeros(c["n"], dtype=bool)
        for s, T in zip(c["start"], c["length"]):
            live[s:s + T] = True
        assert not live[0] and not live[-1] and np.count_nonzero(~live) == 2 * len(c["start"]) + 1
        assert np.all(np.isnan(Y[~live]))
    if name == "G":
        torch, k, d = ctx()
        rows = k.gv_chunk_rows(c["n"])
        assert c["n"] == 2 * rows + 37 and rows == amd.convert.gv_chunk_rows(c["n"])
    Y2, none = gpu_ascend(c, with_trace=False)                                        # without a trace: the same rows
    assert none is None and np.array_equal(Y, Y2, equal_nan=True)


def test_single_row_is_frozen_and_two_rows_are_not(amd):
    c = V.case("D1")                                                                  # n = 1: N < 2
    Y, trace = gpu_ascend(c)
    assert np.array_equal(Y, c["y_ml"])                                               # bit for bit
    check("D1", c, Y, trace)
    assert np.all(trace == trace[0])                                                  # every entry L_d(y_ML)
    c = V.case("D2")
    Y, trace = gpu_ascend(c)
    check("D2", c, Y, trace)
    assert not np.array_equal(Y, c["y_ml"])
    torch, k, d = ctx()
    t = torch.zeros(64, dtype=torch.float64, device=d)
    i = torch.zeros(4, dtype=torch.int64, device=d)
    with pytest.raises(RuntimeError, match="error -1"):                               # n_runs > n
        k.gv_ascend(t, t, 1, 1, 2, i, i, 2, t, t, 1, t, t, None)


def test_constant_column_is_frozen(amd):
    c = V.case("F")
    Y, trace = gpu_ascend(c)
    check("F", c, Y, trace)
    assert np.array_equal(Y[:, 1], c["y_ml"][:, 1]) and np.all(Y[:, 1] == 0.75)       # bit for bit
    assert np.all(trace[:, 1] == trace[0, 1])
    assert not np.array_equal(Y[:, 0], c["y_ml"][:, 0]) and not np.array_equal(Y[:, 2], c["y_ml"][:, 2])


def test_no_sweep_is_the_scaled_start(amd):
    c = V.case("H")
    assert c["iters"] == 0
    Y, trace = gpu_ascend(c)
    assert trace.shape == (1, c["dy"])
    check("H", c, Y, trace)
    v = V.variance(Y)
    assert np.abs(v - c["gv_mean"]).max() <= 1e-12 * c["gv_mean"].max()               # the start has the target's variance


def test_bad_arguments_are_error_codes(amd):
    torch, k, d = ctx()
    t = torch.ones(4096, dtype=torch.float64, device=d)
    i = torch.zeros(4, dtype=torch.int64, device=d)
    one = torch.ones(4, dtype=torch.int64, device=d)

    def call(P=t, r=t, n=1, dy=1, span=1, start=i, length=one, n_runs=1, mean=t, prec=t, iters=1, work=t, Y=t):
        return lambda: k.gv_ascend(P, r, n, dy, span, start, length, n_runs, mean, prec, iters, work, Y, None)
    bad = (call(P=None), call(r=None), call(mean=None), call(prec=None), call(work=None), call(Y=None), call(n=0),
           call(dy=0), call(dy=65), call(span=0), call(span=9), call(n_runs=-1), call(n_runs=2), call(start=None),
           call(length=None), call(iters=-1), call(iters=10001))
    for j, f in enumerate(bad):
        with pytest.raises(RuntimeError, match="error -1"):
            f()
            print("case", j, "returned no error")
    assert k.gv_work_len(1, 65, 1) == -1 and k.gv_chunk_rows(0) == -1
    for n, dy, span in ((1, 1, 1), (165, 2, 2), (761, 17, 2), (60000, 24, 2)):
        assert k.gv_work_len(n, dy, span) == amd.convert.gv_work_len(n, dy, span)
        assert k.gv_chunk_rows(n) == amd.convert.gv_chunk_rows(n)
    Y = torch.full((4, 1), np.nan, dtype=torch.float64, device=d)
    k.gv_ascend(t, t, 4, 1, 2, None, None, 0, t, t, 3, t, Y, None)                    # no runs: valid, nothing is written
    assert bool(torch.isnan(Y).all())


# ---- end to end
def test_trained_map_with_gv_against_the_model(amd):
    import test_gpu_gmm as TG
    from test_gpu_mlpg import c_of
    CA, CB, X, Yp, M, span = R.dynamic_case()
    stats = amd.gv_statistics([CB], rel_std=0.15)
    conv = amd.conversion_train(X, Yp, M, span=span, iters=6, tol=0.0, gv=stats)
    assert np.array_equal(conv["gv_mean"], stats["gv_mean"]) and np.array_equal(conv["gv_prec"], stats["gv_prec"])
    dx, dys = 8, 4
    out, trace = amd.conversion_trajectory(conv, CA, trace=True)
    plain = amd.conversion_trajectory(conv, CA, gv=False)
    keep = ~np.isneginf(CA[:, 0])
    assert out.shape == plain.shape and trace.shape == (31, dys) and np.all(np.isfinite(trace))
    assert np.array_equal(out[:, 0], CA[:, 0]) and np.all(out[~keep, 1:] == 0.0)
    conv = amd.check_conversion(conv)
    start, length = R.runs_of(keep)
    cstart = np.concatenate(([0], np.cumsum(length)[:-1])).astype(np.int64)
    res = {}
    for dtype in (np.float64, LD):                                                    # the same float64 map in both
        full, P, r, gamma = R.trajectory_inputs(conv, CA, span, dtype)
        y_ml = R.solve(P, r, span, cstart, length, dtype)
        sys = V.bands(P, r, span, cstart, length, dtype)                              # as solve: P and r through float64
        res[dtype] = V.ascend(sys, len(P), span, conv["gv_mean"], conv["gv_prec"], 30, y_ml, dtype)[0]
        if dtype is np.float64:
            P0, r0, g0 = P, r, gamma
    t64, tld = res[np.float64], res[LD]
    Xc = R.select(R.dynamic_rows(CA, span)[keep], 5, False) - conv["zbar"][:dx]
    mu_c = conv["means"] - conv["zbar"]
    bar_gamma = TG.estep_bars(Xc, mu_c[:, :dx], np.tril(conv["Wx"]), conv["kx"])[5]
    bar_r = TG.regress_bar(Xc, g0, conv["py"][:, :, None] * conv["A"], conv["py"] * (conv["b"] + conv["zbar"][dx:]))
    e_in = float((bar_gamma.astype(np.float64) / np.maximum(g0, 1e-300)).clip(max=1.0).max() * M
                 + bar_r.astype(np.float64).max() / np.abs(r0).max())
    got = out[keep, 1:]
    worst = 0.0
    for s, T in zip(cstart, length):
        for d in range(dys):
            Rm, _ = R.system(P0[s:s + T], r0[s:s + T], span, d)
            floor = float(np.linalg.cond(Rm)) * (2 * c_of(span) * 2.0 ** -53 + e_in) * np.linalg.norm(t64[s:s + T, d])
            model = np.linalg.norm((t64[s:s + T, d] - tld[s:s + T, d]).astype(np.float64))
            err = np.linalg.norm(got[s:s + T, d] - t64[s:s + T, d])
            assert err <= max(100.0 * model, floor), (int(s), int(T), d, err, model, floor)
            worst = max(worst, err / max(100.0 * model, floor))
    v_ml, v_gv = V.variance(plain[keep, 1:]), V.variance(got)
    print("gv end to end: |gpu - model| / bar <= %.3g; v / gv_mean %s -> %s"
          % (worst, np.round(v_ml / conv["gv_mean"], 3), np.round(v_gv / conv["gv_mean"], 3)))
    record_measurement("gv_trajectory", err_over_bar=worst, err=float(np.abs(got - t64).max()),
                       model_diff=float(np.abs(t64 - tld).max()), v_ml_over_mean=list(v_ml / conv["gv_mean"]),
                       v_gv_over_mean=list(v_gv / conv["gv_mean"]))
    assert np.all(np.abs(v_gv - conv["gv_mean"]) < np.abs(v_ml - conv["gv_mean"]))


def test_step_case_with_gv(amd):
    conv, C = R.step_case()
    mu = np.array([np.var([-1.0, 1.0])])                                              # the variance of the two static means
    gv = dict(gv_mean=mu, gv_prec=1.0 / (0.15 * mu) ** 2)
    plain = amd.conversion_trajectory(conv, C)
    out, trace = amd.conversion_trajectory(conv, C, gv=gv, trace=True)
    v0, v1 = float(np.var(plain[:, 1])), float(np.var(out[:, 1]))
    rough0, rough1 = float(np.abs(np.diff(plain[:, 1])).max()), float(np.abs(np.diff(out[:, 1])).max())
    print("step case: v %.6g -> %.6g (gv_mean 1), largest adjacent step %.6g -> %.6g" % (v0, v1, rough0, rough1))
    record_measurement("gv_step_case", v_ml=v0, v_gv=v1, roughness_ml=rough0, roughness_gv=rough1)
    assert abs(rough0 - R.STEP_ROUGHNESS) <= 1e-9
    assert abs(v1 - 1.0) < abs(v0 - 1.0) and np.array_equal(out[:, 0], C[:, 0])
    full, P, r, _ = R.trajectory_inputs(conv, C, 1)
    y_ml = R.solve(P, r, 1, [0], [len(C)])
    ref = V.ascend(V.bands(P, r, 1, [0], [len(C)]), len(C), 1, gv["gv_mean"], gv["gv_prec"], 30, y_ml)[0]
    assert np.abs(out[:, 1] - ref[:, 0]).max() <= 1e-9
    stored = dict(conv, **gv)                                                         # the same through the map's fields
    assert np.array_equal(amd.conversion_trajectory(stored, C), out)
    assert np.array_equal(amd.conversion_trajectory(stored, C, gv_iters=0),
                          amd.conversion_trajectory(conv, C, gv=gv, gv_iters=0))


def test_without_gv_the_rows_are_the_parents_bit_for_bit(amd):
    """conversion_trajectory on a map without the fields, with gv=False, and with gv=False on a map that carries them,
    against the rows of the commit before the global-variance term existed: sha256 digests recorded on the MI355X at the
    commit tests/golden/gv_parent_digests.json names (tests/gv_parent_cases.py)."""
    import json
    import gv_parent_cases as P
    with open(P.FIXTURE) as f:
        want = json.load(f)["cases"]
    cases = P.cases()
    assert set(cases) == set(want) == {"step", "step_gap", "dynamic"}
    bad = []
    for name, (conv, C) in cases.items():
        dys = int(conv["dy"]) // 2
        stored = dict(conv, gv_mean=np.full(dys, 1.5), gv_prec=np.full(dys, 30.0))
        got = dict(plain=P.rows(amd, conv, C), off=P.rows(amd, conv, C, gv=False), stored_off=P.rows(amd, stored, C, gv=False))
        bad += ["%s.%s" % (name, k) for k, v in got.items() if P.digest(v) != want[name]]
        assert P.digest(P.rows(amd, stored, C)) != want[name], name                   # and with the term they do move
    assert not bad, bad
