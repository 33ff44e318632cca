"""The conditional E-step and the EM refinement of the mixture sequence on the MI355X (convert.conversion_trajectory_em ->
eaqhm_mlpg_estep with eaqhm_gmm_regress, eaqhm_mlpg_solve, eaqhm_gv_ascend) against the NumPy model of DESIGN.md §12.4
(tests/mlpg_em_ref.py) in np.longdouble.  Hand-built inputs only.

Bars (u = 2^-53, ulp = 2^-52, L the span, dx the source columns, 2 dy the target columns with their deltas; every bar is
TWICE a worst-case rounding bound computed in long double from absolute values, plus the allowances for the library
functions named below, which are test_gpu_gmm.py's).

lp.  The static half of Yd is the trajectory itself: exact.  The delta half is eaqhm_ceps_delta's sum: w_tau = tau / den
carries one rounding, c_+ - c_- one, the product and the addition are one fma, L terms are added: |dYd_j| <= eD_j =
(L + 3) u sum_tau |w_tau| (|c_+| + |c_-|) (test_gpu_mlpg.py).  E_j = bq_j + sum_k A_jk x_k is dx products summed in some
order and one addition: |dE_j| <= eE_j = (dx + 2) u (|bq_j| + sum_k |A_jk| |x_k|).  The residual d_j = Yd_j - E_j adds its
own rounding: |dd_j| <= ed_j = eD_j + eE_j + u (|d_j| + eD_j + eE_j).  q = sum_j py_j d_j^2: the squares of the perturbed
residuals differ by at most 2 |d_j| ed_j + ed_j^2, and the weighted sum of squares costs two roundings per term (py_j d_j,
then the fma) and at most 2 dy additions: (2 dy + 2) u sum_j py_j (|d_j| + ed_j)^2; eq is the sum of both.
lp = (ln pi + kc) - q / 2: two additions, u |ln pi + kc| + u |lp|, and the device's log behind ln pi, 4 ulp of |ln pi|:
    bar_lp = 2 (eq / 2 + u |ln pi + kc| + u |lp|) + 4 ulp |ln pi|.
It is checked directly where M = 1 (ll = lp) and enters the other two.

ll = max + ln sum_m exp(lp_m - max).  When the lp move by at most bar_lp_m each, ll moves by at most
ln sum_m gamma_m exp(bar_lp_m) (sum_m exp(lp_m + b_m) = exp(ll) sum_m gamma_m exp(b_m); the lower side is no larger by
Cauchy-Schwarz): a component far below the others does not count with its own, large, bar.  Components whose gamma is 0
in long double (a zero prior, or more than 11 000 nepers below) are left out of it.  Evaluating it adds, relative to the
sum s, 4 ulp for exp, one for the rounding of lp - max and (M - 1) u for the additions, then 4 ulp of |ln s| <= ln M for
log and u |ll| for the last addition: bar_ll = ln sum_m gamma_m exp(bar_lp_m) + 2 (ulp (5 + M / 2 + 4 ln M) + u |ll|).
gamma_m = exp(lp_m - max) / s: its relative error is expm1 of the absolute error of lp_m - ll, at most bar_lp_m + bar_ll,
plus 4 ulp for exp and one for the quotient: bar_gamma = gamma (expm1(bar_lp_m + bar_ll) + 5 ulp) + 2^-1070 (below
2^-1022 a double has fewer bits).

The loop (conversion_trajectory_em against the model's refine): 100 x the model's own float64-to-long-double difference
per quantity, floored at the one-step bars (§12's rule, test_gpu_mlpg.py): the posteriors at bar_gamma above, the mean
log-likelihood at the mean of bar_ll, the trajectory per system at cond_2(R) x (the solve's backward bar + the relative
one-step bars of the posteriors and of the regression, which perturb P and r) x ||y||_2.

Measured on the MI355X (profiles/mlpg_em/parity_measurements.json): ll at most 0.089 and gamma at most 0.070 of their bars
over the nine shapes; the hand case 5.6e-16 from the model's y and its mean log-likelihood at 0.0013 of the bar; the
dynamic case's trajectory at 6.8e-5, its posteriors at 0.022 and its trace at 0.004 of their bars (the trajectory 8.7e-15
from the model, whose own difference is 4.3e-15), with the global-variance term on top at 3.5e-4."""
import math

import numpy as np
import pytest

import gv_ref as V
import mlpg_em_ref as E
import mlpg_ref as R
from conftest import record_measurement

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = LD(2.0) ** -53
ULP = LD(2.0) ** -52


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


def gpu_estep(p, launches=2):
    """(gamma [n, M], ll [n]) of a problem dict, both filled with NaN before the launch, from launches that must agree bit
    for bit."""
    torch, c, d = ctx()
    n, M = p["prior"].shape
    dx, dy = p["X"].shape[1], p["Y"].shape[1]
    out = []
    for _ in range(launches):
        gamma = torch.full((n, M), np.nan, dtype=torch.float64, device=d)
        ll = torch.full((n,), np.nan, dtype=torch.float64, device=d)
        c.mlpg_estep(dev(p["X"]), dev(p["prior"]), dev(p["A"]), dev(p["bq"]), dev(p["py"]), dev(p["kc"]), dev(p["Y"]), n, dx,
                     dy, M, p["span"], dev(p["start"], np.int64), dev(p["length"], np.int64), len(p["start"]), gamma, ll)
        out.append((gamma.cpu().numpy(), ll.cpu().numpy()))
    for g, l in out[1:]:
        assert np.array_equal(g, out[0][0], equal_nan=True) and np.array_equal(l, out[0][1], equal_nan=True)
    return out[0]


# ---- run tables
def small_runs(L, limit):
    """Runs of 1, 2, 2 L and 2 L + 1 rows from row 0 on, a row that belongs to no run after each, as many as end before
    row `limit`: ([start], [length], the first free row)."""
    start, length, t = [], [], 0
    for T in (1, 2, 2 * L, 2 * L + 1):
        if t + T + 1 > limit:
            break
        start.append(t)
        length.append(T)
        t += T + 1
    return start, length, t


def run_table(n, L, mode):
    """(start, length) int64.  'plain': the small runs, then one to row n - 1.  'adjacent' (n >= 65): the small runs, one
    that ends at row 63, one that starts at row 64 (4 L + 1 rows when a gap and a last run to row n - 1 fit behind it).
    'crossing': the small runs, one of 4 L + 1 rows centred on row 64, a gap, one to row n - 1."""
    if mode == "plain":
        start, length, t = small_runs(L, n - 1)
        start, length = start + [t], length + [n - t]
    elif mode == "adjacent":
        start, length, t = small_runs(L, 63)
        start, length = start + [t], length + [64 - t]
        if n >= 64 + 4 * L + 1 + 2:
            start, length = start + [64, 64 + 4 * L + 2], length + [4 * L + 1, n - (64 + 4 * L + 2)]
        else:
            start, length = start + [64], length + [n - 64]
    else:
        start, length, t = small_runs(L, 64 - 2 * L)
        a = 64 - 2 * L
        start, length = start + [a, a + 4 * L + 2], length + [4 * L + 1, n - (a + 4 * L + 2)]
    start, length = np.array(start, dtype=np.int64), np.array(length, dtype=np.int64)
    assert np.all(length >= 1) and start[0] == 0 and start[-1] + length[-1] == n
    assert np.all(start[1:] >= start[:-1] + length[:-1])                             # disjoint and ascending
    return start, length


def live_rows(n, start, length):
    live = np.zeros(n, dtype=bool)
    for s, T in zip(start, length):
        live[s:s + T] = True
    return live


# ---- problems
def problem(n, dx, dy, M, L, mode, seed, special=False):
    """A seeded problem dict.  Priors with exact zeros where M > 1.  With `special` (tables that open with a run of one
    row): row 0 is lost (Y = 1e200) and the middle row of the last run has Y = 1e6, which puts its components more than
    800 nepers apart."""
    rng = np.random.default_rng(seed)
    start, length = run_table(n, L, mode)
    X = rng.standard_normal((n, dx))
    prior = rng.uniform(0.05, 1.0, (n, M)) ** 3
    if M > 1:
        zero = rng.uniform(size=(n, M)) < 0.2
        zero[np.arange(n), rng.integers(0, M, n)] = False                             # a row keeps a component
        prior[zero] = 0.0
    prior /= prior.sum(axis=1, keepdims=True)
    A = rng.standard_normal((M, 2 * dy, dx)) * 0.5 / math.sqrt(dx)
    bq = rng.standard_normal((M, 2 * dy)) * 0.5
    py = np.exp(rng.uniform(-1.0, 1.0, (M, 2 * dy)))
    kc = 0.5 * np.log(py).sum(axis=1) - dy * math.log(2.0 * math.pi)
    Y = rng.standard_normal((n, dy))
    p = dict(X=X, prior=prior, A=A, bq=bq, py=py, kc=kc, Y=Y, span=L, start=start, length=length, n=n)
    if special:
        assert length[0] == 1 and M > 1
        Y[0] = 1e200
        p["lost"] = 0
        p["far"] = int(start[-1] + length[-1] // 2)
        Y[p["far"]] = 1e6 * np.where(rng.uniform(size=dy) < 0.5, -1.0, 1.0)
        prior[p["far"]] = 1.0 / M                                                     # every component is in the row
    return p


def estep_bars(p):
    """(lp, ll, gamma of the long-double model; bar_lp [n, M], bar_ll [n], bar_gamma [n, M]) as the docstring derives; NaN
    on the rows outside every run."""
    X, prior, A, bq, py, kc, Y = (np.asarray(p[k], dtype=np.float64).astype(LD) for k in ("X", "prior", "A", "bq", "py", "kc", "Y"))
    L, start, length = p["span"], p["start"], p["length"]
    n, M = prior.shape
    dx, dy = X.shape[1], Y.shape[1]
    lp, ll, gamma = E.estep(X, prior, A, bq, py, Y, L, start, length, LD, kc=kc)
    Yd = E.dynamic_target(Y, L, start, length, LD)
    live = ~np.isnan(Yd[:, 0])
    eD = np.zeros((n, 2 * dy), dtype=LD)
    w = R.window(L, LD)
    for s, T in zip(start, length):
        c, idx = np.abs(Y[s:s + T]), np.arange(T)
        for tau in range(1, L + 1):
            eD[s:s + T, dy:] += w[tau - 1] * (c[np.minimum(idx + tau, T - 1)] + c[np.maximum(idx - tau, 0)])
    eD *= (L + 3) * U
    bar_lp = np.full((n, M), np.nan, dtype=LD)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        lnpi = np.log(prior)
        for m in range(M):
            d = np.abs(Yd - (X @ A[m].T + bq[m]))
            eE = (dx + 2) * U * (np.abs(X) @ np.abs(A[m]).T + np.abs(bq[m]))
            ed = eD + eE + U * (d + eD + eE)
            eq = (py[m] * (2 * d * ed + ed * ed)).sum(axis=1) + (2 * dy + 2) * U * (py[m] * (d + ed) ** 2).sum(axis=1)
            bar_lp[:, m] = 2 * (eq / 2 + U * np.abs(lnpi[:, m] + kc[m]) + U * np.abs(lp[:, m])) + 4 * ULP * np.abs(lnpi[:, m])
        counted = np.where(gamma > 0, gamma * np.exp(np.where(gamma > 0, bar_lp, 0)), 0)
        move = np.log(counted.sum(axis=1))
        bar_ll = move + 2 * (ULP * (5 + LD(M) / 2 + 4 * np.log(LD(M))) + U * np.abs(ll))
        bar_gamma = gamma * (np.expm1(np.where(gamma > 0, bar_lp, 0) + bar_ll[:, None]) + 5 * ULP) + LD(2.0) ** -1070
    bar_ll[~live], bar_gamma[~live] = np.nan, np.nan
    return lp, ll, gamma, bar_lp, bar_ll, bar_gamma


# ---- 1. the kernel against the long-double model
CASES = (   # n, dx, dy, M, span, table, the special rows
    (1, 2, 1, 1, 1, "plain", False),
    (63, 6, 3, 2, 2, "plain", False),
    (64, 34, 17, 9, 8, "plain", False),
    (65, 64, 32, 64, 1, "adjacent", False),
    (130, 6, 3, 9, 2, "adjacent", True),
    (130, 64, 32, 64, 8, "crossing", True),
    (130, 34, 17, 2, 8, "adjacent", True),
    (130, 2, 1, 9, 1, "crossing", True),
    (130, 6, 3, 1, 2, "crossing", False),
)


def test_the_cases_cover_the_axes_and_the_run_shapes():
    assert {c[0] for c in CASES} == {1, 63, 64, 65, 130}
    assert {c[1:3] for c in CASES} == {(2, 1), (6, 3), (34, 17), (64, 32)}
    assert {c[3] for c in CASES} == {1, 2, 9, 64} and {c[4] for c in CASES} == {1, 2, 8}
    for L in (1, 2, 8):
        tables = [run_table(n, L, mode) for n, _, _, _, span, mode, _ in CASES if span == L]
        lengths = set(int(T) for _, length in tables for T in length)
        assert {1, 2, 2 * L, 2 * L + 1, 4 * L + 1} <= lengths, (L, lengths)
        for n, _, _, _, span, mode, _ in CASES:
            if span != L or n < 130:
                continue
            start, length = run_table(n, L, mode)
            end = start + length
            assert not live_rows(n, start, length).all()                             # rows outside every run
            if mode == "adjacent":
                assert 64 in end and 64 in start                                     # one ends at row 63, the next starts at 64
            else:
                assert np.any((start < 64) & (end > 65))                             # one crosses row 64
    assert any(c[5] == "adjacent" and c[0] == 130 for c in CASES) and any(c[5] == "crossing" for c in CASES)
    s65, l65 = run_table(65, 1, "adjacent")
    assert s65[-1] == 64 and l65[-1] == 1 and s65[-2] + l65[-2] == 64


@pytest.mark.parametrize("n,dx,dy,M,L,mode,special", CASES)
def test_estep_against_long_double(amd, n, dx, dy, M, L, mode, special):
    p = problem(n, dx, dy, M, L, mode, 7 * n + 100 * dx + M + L, special)
    gamma, ll = gpu_estep(p)
    lp_r, ll_r, gamma_r, bar_lp, bar_ll, bar_gamma = estep_bars(p)
    live = live_rows(n, p["start"], p["length"])
    assert np.all(np.isnan(gamma[~live])) and np.all(np.isnan(ll[~live]))            # rows outside the runs keep their NaN
    assert not np.any(np.isnan(gamma[live])) and not np.any(np.isnan(ll[live]))
    check = live.copy()
    if special:
        lost, far = p["lost"], p["far"]
        assert np.isneginf(ll[lost]) and np.array_equal(gamma[lost], p["prior"][lost])     # the lost row: no preference
        assert np.isneginf(ll_r[lost])
        check[lost] = False
        top = np.sort(lp_r[far].astype(np.float64))
        assert top[-1] - top[-2] > 800.0
        assert np.isfinite(ll[far]) and sorted(set(gamma[far])) == [0.0, 1.0] and gamma[far].sum() == 1.0
        assert int(np.argmax(gamma[far])) == int(np.argmax(lp_r[far]))
    if M > 1:
        assert np.all(gamma[live][p["prior"][live] == 0.0] == 0.0)                    # a zero prior: exactly 0
        assert np.any(p["prior"][live] == 0.0)
    else:
        assert np.all(gamma[live] == 1.0)
        assert np.all(np.abs(ll[check].astype(LD) - lp_r[check, 0]) <= bar_lp[check, 0])     # ll is lp itself
    e_ll = np.abs(ll[check].astype(LD) - ll_r[check])
    e_g = np.abs(gamma[check].astype(LD) - gamma_r[check])
    worst_ll = float((e_ll / bar_ll[check]).max()) if check.any() else 0.0
    worst_g = float((e_g / bar_gamma[check]).max()) if check.any() else 0.0
    print("mlpg estep (%d, %d, %d, %d, %d, %s): |dll| / bar <= %.3g, |dgamma| / bar <= %.3g, max |dll| %.3g"
          % (n, dx, dy, M, L, mode, worst_ll, worst_g, float(e_ll.max()) if check.any() else 0.0))
    record_measurement("mlpg_em_estep_%d_%d_%d_%d_%d" % (n, dx, dy, M, L), ll_err_over_bar=worst_ll,
                       gamma_err_over_bar=worst_g, ll_err=float(e_ll.max()) if check.any() else 0.0,
                       gamma_err=float(e_g.max()) if check.any() else 0.0)
    assert np.all(np.isfinite(ll[check])) and np.all(np.isfinite(gamma[live]))
    assert np.all(e_ll <= bar_ll[check])
    assert np.all(e_g <= bar_gamma[check])
    assert np.all(np.abs(gamma[check].sum(axis=1) - 1.0) <= M * 2.0 ** -52)


def test_bad_arguments_are_error_codes(amd):
    torch, c, d = ctx()
    t = torch.ones(4096, dtype=torch.float64, device=d)
    i = torch.zeros(4, dtype=torch.int64, device=d)
    one = torch.ones(4, dtype=torch.int64, device=d)
    o = torch.zeros(8, dtype=torch.float64, device=d)
    good = [t, t, t, t, t, t, t, 1, 1, 1, 1, 1, i, one, 1, o, o[4:]]
    c.mlpg_estep(*good)                                                               # the template itself is valid

    def changed(k, v):
        a = list(good)
        a[k] = v
        return a
    bad = [changed(k, None) for k in (0, 1, 2, 3, 4, 5, 6, 12, 13, 15, 16)]
    bad += [changed(7, 0), changed(8, 0), changed(8, 65), changed(9, 0), changed(9, 33), changed(10, 0), changed(10, 65),
            changed(11, 0), changed(11, 9), changed(14, -1), changed(14, 2)]
    for k, a in enumerate(bad):
        with pytest.raises(RuntimeError, match="error -1"):
            c.mlpg_estep(*a)
            print("case", k, "returned no error")
    g = torch.full((4, 1), np.nan, dtype=torch.float64, device=d)
    c.mlpg_estep(t, t, t, t, t, t, t, 4, 1, 1, 1, 2, None, None, 0, g, g)             # no runs: valid, nothing is written
    assert bool(torch.isnan(g).all())


# ---- 2. the same bits wherever the run lies
def test_a_run_gives_the_same_bits_wherever_it_lies(amd):
    rng = np.random.default_rng(77)
    T, dx, dy, M, L, n = 29, 6, 3, 9, 2, 130
    base = problem(T, dx, dy, M, L, "plain", 78)
    rows = {k: base[k] for k in ("X", "prior", "Y")}
    got = []
    for at in (0, 1, 37):                                                             # 37: the run crosses row 64
        p = problem(n, dx, dy, M, L, "plain", 79 + at)
        for k in ("A", "bq", "py", "kc"):
            p[k] = base[k]
        for k, v in rows.items():
            p[k][at:at + T] = v
        start, length = [at], [T]
        if at > 1:
            start, length = [0] + start, [at - 1] + length                            # other runs around it, and gaps
        if at == 1:
            p["Y"][0] = rng.standard_normal(dy) * 1e3                                  # a neighbour outside the run: not read
        start, length = start + [at + T + 1], length + [n - (at + T + 1)]
        p["start"], p["length"] = np.array(start, dtype=np.int64), np.array(length, dtype=np.int64)
        gamma, ll = gpu_estep(p)
        assert np.isnan(ll[at + T]) and not np.any(np.isnan(ll[at:at + T]))
        got.append((gamma[at:at + T], ll[at:at + T]))
    for g, l in got[1:]:
        assert np.array_equal(g, got[0][0]) and np.array_equal(l, got[0][1])
    ref = estep_bars(dict(base, start=np.array([0]), length=np.array([T])))
    assert np.all(np.abs(got[0][1].astype(LD) - ref[1]) <= ref[4])


# ---- 3. fixed points through the host path
def model_map(f, span):
    from test_gpu_mlpg import model_map as mm
    return mm(f, span)


def one_component_map():
    rng = np.random.default_rng(4)
    T, d, span = 90, 2, 2
    CA = np.hstack((np.full((T, 1), -3.0), np.cumsum(rng.standard_normal((T, d)), axis=0) * 0.3))
    CB = np.hstack((np.full((T, 1), -2.0), CA[:, 1:] @ rng.standard_normal((d, d)) + 0.1 * rng.standard_normal((T, d))))
    CA[[17, 18, 70]] = (-np.inf, 0.0, 0.0)
    keep = CA[:, 0] > -np.inf
    f = R.train(R.dynamic_rows(CA, span)[keep], R.dynamic_rows(CB, span)[keep], 1, iters=2)
    return model_map(f, span), CA


def test_fixed_points(amd):
    from eaqhm_amd.convert import conversion_trajectory_em
    conv, CA = one_component_map()
    plain = amd.conversion_trajectory(conv, CA)
    out, ll = conversion_trajectory_em(conv, CA, em_iters=3, em_trace=True)
    assert np.array_equal(out, plain) and ll.shape == (4,) and np.all(ll == ll[0]) and np.isfinite(ll[0])
    assert np.array_equal(conversion_trajectory_em(conv, CA, em_iters=3), plain)
    conv, C = R.step_case()
    assert np.array_equal(conversion_trajectory_em(conv, C, em_iters=3), amd.conversion_trajectory(conv, C))


def test_no_iteration_is_conversion_trajectory_bit_for_bit(amd):
    from eaqhm_amd.convert import conversion_trajectory_em
    conv, C = E.ambiguous_case()
    holed = C.copy()
    holed[[0, 20, 21]] = (-np.inf, 0.0)
    mu = np.array([0.9])
    gv = dict(gv_mean=mu, gv_prec=1.0 / (0.15 * mu) ** 2)
    with_gv = dict(conv, **gv)
    for rows in (C, holed):
        assert np.array_equal(conversion_trajectory_em(conv, rows, em_iters=0), amd.conversion_trajectory(conv, rows))
        assert np.array_equal(conversion_trajectory_em(conv, rows, em_iters=0, gv=gv), amd.conversion_trajectory(conv, rows, gv=gv))
        assert np.array_equal(conversion_trajectory_em(with_gv, rows, em_iters=0), amd.conversion_trajectory(with_gv, rows))
        assert np.array_equal(conversion_trajectory_em(with_gv, rows, em_iters=0, gv=False), amd.conversion_trajectory(conv, rows))
        a, ta = conversion_trajectory_em(conv, rows, em_iters=0, gv=gv, gv_iters=7, trace=True)
        b, tb = amd.conversion_trajectory(conv, rows, gv=gv, gv_iters=7, trace=True)
        assert np.array_equal(a, b) and np.array_equal(ta, tb) and ta.shape == (8, 1)
        a, ta, la = conversion_trajectory_em(conv, rows, em_iters=0, em_trace=True, gv=gv, gv_iters=7, trace=True)
        assert np.array_equal(a, b) and np.array_equal(ta, tb) and la.shape == (1,)  # scoring the start changes nothing


# ---- 4. the loop against the model
def loop_bars(g, C, span, iters):
    """Per iteration i = 0 .. iters the mean of bar_ll at the model's y^(i); and the estep_bars of the last E-step that
    feeds an M-step (at y^(iters - 1)), with the problem dict it was computed on."""
    k = E.inputs(g, C, span)
    n = len(k["X"])
    means, last = [], None
    for i in range(iters + 1):
        st = E.refine(g, C, span, i, state=True)[3]
        kc = 0.5 * np.log(k["py"]).sum(axis=1) - (k["py"].shape[1] // 2) * math.log(2.0 * math.pi)   # the host's numbers
        p = dict(X=k["X"], prior=k["prior"], A=k["A"], bq=k["bq"], py=k["py"], kc=kc, Y=st["Y"],
                 span=span, start=k["start"], length=k["length"], n=n)
        bars = estep_bars(p)
        means.append(float(bars[4].mean()))
        if i == iters - 1:
            last = (p, bars)
    return np.array(means), last


def test_ambiguous_case(amd):
    from eaqhm_amd.convert import conversion_trajectory_em
    conv, C = E.ambiguous_case()
    n = len(C)
    out, ll = conversion_trajectory_em(conv, C, em_iters=3, em_trace=True)
    o64, t64, _ = E.refine(conv, C, 1, 3)
    _, tld, _ = E.refine(conv, C, 1, 3, LD)
    assert np.abs(out[:, 1] - o64[:, 1]).max() <= 1e-9 and np.abs(out[:, 1] - E.HAND_Y[3]).max() <= 1e-9
    assert np.array_equal(out[:, 0], C[:, 0])
    first = amd.conversion_trajectory(conv, C)
    assert np.abs(first[:, 1] - 0.2).max() <= 1e-12
    floors, _ = loop_bars(conv, C, 1, 3)
    own = np.abs(t64.astype(LD) - tld).astype(np.float64) / n
    err = np.abs(ll - t64 / n)
    bar = np.maximum(100.0 * own, floors)
    print("ambiguous case: mean log-likelihood %s, |gpu - model| %s, bar %s" % (ll, err, bar))
    record_measurement("mlpg_em_ambiguous", y_err=float(np.abs(out[:, 1] - o64[:, 1]).max()), loglik=list(ll),
                       loglik_err_over_bar=float((err / bar).max()), model_diff=float(own.max()))
    assert ll.shape == (4,) and np.all(err <= bar)
    _, t6, _ = E.refine(conv, C, 1, 6)
    stop = E.stop_iteration(t6, n, 1e-3, 6)
    assert stop == 3
    out_t, ll_t = conversion_trajectory_em(conv, C, em_iters=6, em_tol=1e-3, em_trace=True)
    assert len(ll_t) == stop + 1                                                     # it stops where the model stops
    assert np.array_equal(out_t, out)                                                # ... with the trajectory that E-step scored
    assert np.array_equal(conversion_trajectory_em(conv, C, em_iters=6, em_tol=1e-3), out)


_DYN = {}


def dynamic():
    if not _DYN:
        CA, CB, X, Y, M, span = R.dynamic_case(N=400, d=3, M=3, span=2, seed=31)
        f = R.train(X, Y, M, iters=6, tol=-1.0)
        _DYN.update(CA=CA, CB=CB, M=M, span=span, f=f, conv=model_map(f, span),
                    r64=E.refine(f, CA, span, 4, state=True), rld=E.refine(f, CA, span, 4, LD, state=True))
        _DYN["floors"], _DYN["last"] = loop_bars(f, CA, span, 4)
    return _DYN


def trajectory_check(got, t64, tld, st, span, M, last, tag):
    """Asserts §12's rule per system on compacted rows; returns the worst err / bar."""
    import test_gpu_gmm as TG
    from test_gpu_mlpg import c_of
    p, bars = last
    gamma, bar_gamma = bars[2].astype(np.float64), bars[5].astype(np.float64)
    bar_r = TG.regress_bar(p["X"], gamma, p["py"][:, :, None] * p["A"], p["py"] * p["bq"])
    e_in = float((bar_gamma / np.maximum(gamma, 1e-300)).clip(max=1.0).max() * M
                 + bar_r.astype(np.float64).max() / np.abs(st["r"]).max())
    worst = 0.0
    for s, T in zip(st["start"], st["length"]):
        for d in range(got.shape[1]):
            Rm, _ = R.system(st["P"][s:s + T], st["r"][s:s + T], span, d)
            floor = float(np.linalg.cond(Rm)) * (2 * c_of(span) * 2.0 ** -53 + e_in) * np.linalg.norm(t64[s:s + T, d])
            model = np.linalg.norm((t64[s:s + T, d] - tld[s:s + T, d]).astype(np.float64))
            err = np.linalg.norm(got[s:s + T, d] - t64[s:s + T, d])
            assert err <= max(100.0 * model, floor), (tag, int(s), int(T), d, err, model, floor)
            worst = max(worst, err / max(100.0 * model, floor))
    return worst


def test_dynamic_case(amd):
    from eaqhm_amd import convert
    e = dynamic()
    CA, span, M, conv = e["CA"], e["span"], e["M"], e["conv"]
    (o64, t64, g64, st), (old, tld, gld, _) = e["r64"], e["rld"]
    keep = ~np.isneginf(CA[:, 0])
    n = int(keep.sum())
    out, ll = convert.conversion_trajectory_em(conv, CA, em_iters=4, em_trace=True)
    assert out.shape == o64.shape and np.array_equal(out[:, 0], CA[:, 0]) and np.all(out[~keep, 1:] == 0.0)
    assert np.array_equal(convert.conversion_trajectory_em(conv, CA), out)            # 4 is the default; no trace, same rows
    worst = trajectory_check(out[keep, 1:], o64[keep, 1:], old[keep, 1:], st, span, M, e["last"], "em")
    # the trace
    own = np.abs(t64.astype(LD) - tld).astype(np.float64)
    err = np.abs(ll - t64 / n)
    bar = np.maximum(100.0 * own / n, e["floors"])
    assert ll.shape == (5,) and np.all(err <= bar), (err, bar)
    assert np.all(np.diff(ll) * n >= -100.0 * own[1:])                               # it does not fall: the CPU test's allowance
    # the posteriors of the last M-step: the kernel on the device's own y^(3)
    y3 = convert.conversion_trajectory_em(conv, CA, em_iters=3)[keep, 1:]
    p, bars = e["last"]
    v = convert.check_conversion(conv)
    D = amd.dynamic_rows(CA, span)
    mix = convert._Mixture(convert._dynamic_columns(D[keep], CA.shape[1], 1), v["zbar"][:v["dx"]], M, 0)
    prior, _ = mix.estep((v["means"] - v["zbar"])[:, :v["dx"]], v["Wx"], v["kx"])
    gamma, _ = gpu_estep(dict(p, X=mix.Z.cpu().numpy(), prior=prior.cpu().numpy(), Y=y3), launches=1)
    own_g = float(np.abs(g64.astype(LD) - gld).max())
    err_g = np.abs(gamma - g64)
    bar_g = np.maximum(100.0 * own_g, bars[5].astype(np.float64))
    assert np.all(err_g <= bar_g), float((err_g / bar_g).max())
    moved = float(np.abs(gamma - p["prior"]).max())
    print("dynamic case: trajectory / bar <= %.3g, trace err %s (bar %s), posteriors / bar <= %.3g, moved by %.3g; rises %s"
          % (worst, err, bar, float((err_g / bar_g).max()), moved, np.diff(ll) * n))
    record_measurement("mlpg_em_dynamic", trajectory_err_over_bar=worst, trajectory_err=float(np.abs(out[keep] - o64[keep]).max()),
                       trajectory_model_diff=float(np.abs(o64[keep] - old[keep]).max()),
                       loglik_err_over_bar=float((err / bar).max()), loglik_rises=list(np.diff(ll) * n),
                       posterior_err_over_bar=float((err_g / bar_g).max()), posteriors_moved_by=moved)
    assert moved > 0.5


def test_dynamic_case_with_gv(amd):
    from eaqhm_amd import convert
    e = dynamic()
    CA, span, M, conv = e["CA"], e["span"], e["M"], e["conv"]
    stats = amd.gv_statistics([e["CB"]], rel_std=0.15)
    keep = ~np.isneginf(CA[:, 0])
    out, trace, ll = convert.conversion_trajectory_em(conv, CA, em_iters=4, gv=stats, trace=True, em_trace=True)
    plain, ll_plain = convert.conversion_trajectory_em(conv, CA, em_iters=4, em_trace=True)
    assert trace.shape == (31, 3) and np.all(np.isfinite(trace)) and np.array_equal(ll, ll_plain)
    assert np.array_equal(out[:, 0], CA[:, 0]) and np.all(out[~keep, 1:] == 0.0)
    res = {}
    for dtype, ref in ((np.float64, e["r64"]), (LD, e["rld"])):
        st = ref[3]
        sys = V.bands(st["P"], st["r"], span, st["start"], st["length"], dtype)
        res[dtype] = V.ascend(sys, len(st["P"]), span, stats["gv_mean"], stats["gv_prec"], 30,
                              st["Y"], dtype)[0]
    worst = trajectory_check(out[keep, 1:], res[np.float64], res[LD], e["r64"][3], span, M, e["last"], "em + gv")
    v_em, v_gv = V.variance(plain[keep, 1:]), V.variance(out[keep, 1:])
    print("em + gv: |gpu - model| / bar <= %.3g; v / gv_mean %s -> %s"
          % (worst, np.round(v_em / stats["gv_mean"], 3), np.round(v_gv / stats["gv_mean"], 3)))
    record_measurement("mlpg_em_dynamic_gv", err_over_bar=worst, err=float(np.abs(out[keep, 1:] - res[np.float64]).max()),
                       model_diff=float(np.abs(res[np.float64] - res[LD]).max()))
    assert np.all(np.abs(v_gv - stats["gv_mean"]) < np.abs(v_em - stats["gv_mean"]))
