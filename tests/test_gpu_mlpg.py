"""The delta rows and the trajectory solve on the MI355X (convert.dynamic_rows / conversion_train(span=) /
conversion_trajectory -> eaqhm_ceps_delta, eaqhm_mlpg_solve) against the NumPy model of DESIGN.md §12.1
(tests/mlpg_ref.py) in np.longdouble.  Hand-built inputs only.

Bars (u = 2^-53, L the span; every bar is TWICE a worst-case rounding bound).

Delta rows.  w_tau = tau / den carries one rounding (den = 2 sum k^2 is exact), c_+ - c_- one, the product and the
addition are one fma, and L terms are added: at most (L + 3) u <= (2 L + 2) u relative to sum_tau |w_tau| (|c_+| + |c_-|).
The bar is the issue's: 2 (2 L + 2) u sum_tau |w_tau| (|c_+| + |c_-|) per entry.  Empty rows give exact zeros.

Solve, backward error.  ||R yhat - q||_2 <= 2 c(L) u (||R|| ||yhat||_2 + ||qbar||_2) per system, with R and q formed in
long double from the very P and r given to the kernel, ||R|| := max_i R_ii <= ||R||_2 (a smaller norm is a stricter bar)
and qbar = |r^s| + |W|^T |r^D| >= |q| entry by entry (forming q can cancel, so its rounding is bounded by qbar, not q).
c(L) = (10 L + 9)(4 L + 1), from three parts, b = 2 L the half-bandwidth:
 (a) forming the band.  An entry a of W is a sum of at most L same-signed w_tau (runs of one row: exactly 0):
     |da| <= (L + 1) u |a|.  R_ij = [i = j] P^s_i + sum_u a_ui a_uj P^D_u has at most 2 L + 1 products, each with the two da,
     the rounding of a_ui a_uj and the fma: 2 (L + 1) + 2 <= 2 L + 4 roundings, plus 2 L + 1 additions:
     |dR_ij| <= (4 L + 5) u B_ij, B = diag(P^s) + |W|^T diag(P^D) |W|.  B_ii = R_ii and B_ij <= sqrt(B_ii B_jj) <= max_i R_ii
     (Cauchy-Schwarz), 4 L + 1 entries a row: ||dR||_2 <= ||dR||_inf <= (4 L + 5)(4 L + 1) u ||R||.
     Likewise |dq_i| <= (L + 1 + 2 L + 2) u qbar_i = (3 L + 3) u qbar_i.
 (b) the factorisation R = L D L^T and the two substitutions at half-bandwidth b: (R + E) yhat = q with
     |E| <= gamma_(3 (b + 1) + 1) |L| |D| |L^T| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorems 10.3
     and 10.4 with the inner products of length <= b + 1 of a band; |L||D||L^T| = |G^T||G| for the Cholesky factor G = D^1/2
     L^T).  (|G^T||G|)_ij <= ||g_i|| ||g_j|| = sqrt(R_ii R_jj) <= ||R|| and the band has 2 b + 1 = 4 L + 1 entries a row:
     ||E||_2 <= (6 L + 4)(4 L + 1) u ||R||.
 (c) sum: ((4 L + 5) + (6 L + 4))(4 L + 1) u ||R|| ||yhat|| + (3 L + 3) u ||qbar|| <= c(L) u (||R|| ||yhat|| + ||qbar||).
c(1) = 95, c(2) = 261, c(8) = 2937.  Measured on the MI355X (profiles/mlpg/parity_measurements.json): the residual at most
0.0104 of the bar (0.0105 with ||q|| in place of ||qbar||), the delta rows at most 0.21 of theirs, the forward error at
most 2.7 cond u ||y||, P^D = 0 within 0.49 ulp, the loop's quantities 0.77 to 1.39 x the model's own difference.

Solve, forward error: recorded as a fraction of cond_2(R) u ||y||_2 (evidence, not a bar).

The loop.  100 x the model's own float64-to-long-double difference per quantity, floored at the one-step bars (§12's
rule, test_gpu_gmm.py): the mixture's floors are that file's; py = 1 / v, v = diag(S^yy - A S^xy), moves by py^2 |dv| with
|dv| <= (1 + ||A_d||_1)^2 x the covariance floor; the trajectory moves by at most cond_2(R) x (the backward bar above +
the relative one-step bars of gamma and of the regression, which perturb P and r) x ||y||_2 per system."""
import numpy as np
import pytest

import gmm_ref as G
import mlpg_ref as R
from conftest import record_measurement

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = LD(2.0) ** -53
LONG = 700


def c_of(L):
    return (10 * L + 9) * (4 * L + 1)


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


def gpu_delta(C, span):
    torch, c, d = ctx()
    n, cols = C.shape
    out = torch.full((n, cols), np.nan, dtype=torch.float64, device=d)
    c.ceps_delta(dev(C), n, cols, span, out)
    return out.cpu().numpy()


def gpu_solve(P, r, span, start, length):
    """Y float64[n, dy] filled with NaN before the launch, from two launches that must agree bit for bit."""
    torch, c, d = ctx()
    n, dy = P.shape[0], P.shape[1] // 2
    out = []
    for _ in range(2):
        Y = torch.full((n, dy), np.nan, dtype=torch.float64, device=d)
        work = torch.full((c.mlpg_work_len(n, dy, span),), np.nan, dtype=torch.float64, device=d)
        c.mlpg_solve(dev(P), dev(r), n, dy, span, dev(start, np.int64), dev(length, np.int64), len(start), work, Y)
        out.append(Y.cpu().numpy())
    assert np.array_equal(out[0], out[1], equal_nan=True)                            # the same bits on every run
    return out[0]


# ---- hand-built layouts
def layout(lengths):
    """full bool[n]: runs of these lengths separated by single empty rows; the first touches row 0, the last row n - 1."""
    full = []
    for k, T in enumerate(lengths):
        full += [True] * T + ([False] if k + 1 < len(lengths) else [])
    return np.array(full)


def run_lengths(L, long=LONG):
    return [3, 1, 2 * L + 1, long, 2, 2 * L, 4 * L + 1]


_W = {}


def delta_matrix(T, L):
    if (T, L) not in _W:
        _W[(T, L)] = R.delta_matrix(T, L, LD)
    return _W[(T, L)]


def precisions(n, dy, seed):
    """P, r float64[n, 2 dy]: P^s in [e^-2, e^2], P^D / P^s from 0 (a few rows, and all of column 0 where dy > 1) over
    1e-3 to 1e6 (row by row; the last column at 1e6 throughout)."""
    rng = np.random.default_rng(seed)
    P = np.exp(rng.uniform(-2.0, 2.0, (n, 2 * dy)))
    P[:, dy:] = P[:, :dy] * 10.0 ** rng.uniform(-3.0, 6.0, (n, 1))
    P[:, 2 * dy - 1] = P[:, dy - 1] * 1e6
    P[rng.integers(0, n, size=max(1, n // 50)), dy:] = 0.0
    if dy > 1:
        P[:, dy] = 0.0
    return P, rng.standard_normal((n, 2 * dy)) * P * 3.0


def check_backward(P, r, Y, span, start, length, tag):
    """Asserts the backward bar on every system; returns (worst residual / bar, worst residual / the issue's form)."""
    dy = P.shape[1] // 2
    worst = strict = 0.0
    for s, T in zip(start, length):
        W = delta_matrix(int(T), span)
        Ps, Pd, rs, rd = (a[s:s + T].astype(LD) for a in (P[:, :dy], P[:, dy:], r[:, :dy], r[:, dy:]))
        y = Y[s:s + T].astype(LD)
        assert np.all(np.isfinite(Y[s:s + T])), tag
        q = rs + W.T @ rd
        res = Ps * y + W.T @ (Pd * (W @ y)) - q
        normR = (Ps + (W * W).T @ Pd).max(axis=0)
        qbar = np.abs(rs) + np.abs(W).T @ np.abs(rd)
        n2 = lambda a: np.sqrt((a * a).sum(axis=0))                                   # noqa: E731
        bar = 2 * c_of(span) * U * (normR * n2(y) + n2(qbar))
        assert np.all(n2(res) <= bar), (tag, int(s), int(T))
        worst = max(worst, float((n2(res) / bar).max()))
        strict = max(strict, float((n2(res) / (2 * c_of(span) * U * (normR * n2(y) + n2(q)))).max()))
    return worst, strict


# ---- 1. the delta rows
@pytest.mark.parametrize("span", [1, 2, 8])
@pytest.mark.parametrize("cols", [1, 2, 19, 128])
def test_delta_against_long_double(amd, cols, span):
    full = layout(run_lengths(span, 70))
    n = len(full)
    rng = np.random.default_rng(100 * cols + span)
    C = rng.standard_normal((n, cols)) * 10.0 ** rng.uniform(-2, 2, (n, 1))
    C[~full] = 0.0
    C[~full, 0] = -np.inf
    D = gpu_delta(C, span)
    ref = R.delta_rows(C, span, LD)
    assert np.all(D[~full] == 0.0)                                                    # empty rows: exact zeros
    w = R.window(span, LD)
    mag = np.zeros((n, cols), dtype=LD)
    for s, T in zip(*R.runs_of(full)):
        c, idx = np.abs(C[s:s + T]).astype(LD), np.arange(T)
        for tau in range(1, span + 1):
            mag[s:s + T] += w[tau - 1] * (c[np.minimum(idx + tau, T - 1)] + c[np.maximum(idx - tau, 0)])
    bar = 2 * (2 * span + 2) * U * mag
    err = np.abs(D.astype(LD) - ref)
    worst = float((err[bar > 0] / bar[bar > 0]).max())
    print("delta (cols %d, span %d): |d| / bar <= %.3g" % (cols, span, worst))
    record_measurement("mlpg_delta_%d_%d" % (cols, span), err_over_bar=worst, err=float(err.max()))
    assert np.all(err <= bar)
    s1 = int(np.flatnonzero(R.runs_of(full)[1] == 1)[0])                              # the run of one row: delta exactly 0
    assert np.all(D[R.runs_of(full)[0][s1]] == 0.0)


def test_delta_single_row_and_many_short_runs(amd):
    assert np.all(gpu_delta(np.array([[1.5, -2.0, 3.0]]), 2) == 0.0)                 # n = 1
    assert np.all(gpu_delta(np.array([[-np.inf, 0.0, 0.0]]), 2) == 0.0)
    full = layout([1 + k % 3 for k in range(70)])
    rng = np.random.default_rng(3)
    C = rng.standard_normal((len(full), 5))
    C[~full] = 0.0
    C[~full, 0] = -np.inf
    for span in (1, 2, 8):
        D = gpu_delta(C, span)
        ref = R.delta_rows(C, span, LD)
        assert np.all(D[~full] == 0.0)
        assert np.all(np.abs(D.astype(LD) - ref) <= 2 * (2 * span + 2) * U * 2 * np.abs(C[full]).max() * R.window(span, LD).sum())
    from eaqhm_amd import dynamic_rows
    got = dynamic_rows(C, 2)
    assert got.shape == (len(full), 10) and np.array_equal(got[:, :5], C) and np.array_equal(got[:, 5:], gpu_delta(C, 2))


# ---- 2. the solve
@pytest.mark.parametrize("span", [1, 2, 8])
@pytest.mark.parametrize("dy", [1, 2, 17, 63, 64])
def test_solve_backward_error(amd, dy, span):
    full = layout(run_lengths(span))
    n = len(full)
    start, length = R.runs_of(full)
    assert start[0] == 0 and start[-1] + length[-1] == n and LONG in length
    P, r = precisions(n, dy, 1000 * dy + span)
    Y = gpu_solve(P, r, span, start, length)
    assert np.all(np.isnan(Y[~full]))                                                 # rows outside runs keep their NaN
    worst, strict = check_backward(P, r, Y, span, start, length, (dy, span))
    # forward error (evidence): the short runs, every column; the long run, column dy - 1 (P^D / P^s = 1e6) once per span
    fwd = 0.0
    for s, T in zip(start, length):
        cols = range(dy) if T < LONG else ([dy - 1] if dy == 2 else [])
        for d in cols:
            Rm, q = R.system(P[s:s + T], r[s:s + T], span, d, LD)
            y = R.dense_solve(Rm, q)
            cond = float(np.linalg.cond(Rm.astype(np.float64)))
            e = np.linalg.norm((Y[s:s + T, d].astype(LD) - y).astype(np.float64))
            fwd = max(fwd, e / (cond * float(U) * np.linalg.norm(y.astype(np.float64))))
    print("solve (dy %d, span %d): residual / bar <= %.3g (the issue's form with ||q||: %.3g), forward error <= %.3g "
          "cond u ||y||" % (dy, span, worst, strict, fwd))
    record_measurement("mlpg_solve_%d_%d" % (dy, span), residual_over_bar=worst, residual_over_bar_with_norm_q=strict,
                       forward_error_over_cond_u_norm_y=fwd)


def test_solve_many_short_runs_and_single_row(amd):
    full = layout([1 + k % 3 for k in range(70)])
    start, length = R.runs_of(full)
    assert len(start) == 70
    for span in (1, 2, 8):
        P, r = precisions(len(full), 17, span)
        Y = gpu_solve(P, r, span, start, length)
        assert np.all(np.isnan(Y[~full]))
        check_backward(P, r, Y, span, start, length, ("short", span))
    P, r = precisions(1, 3, 9)                                                        # n = 1
    Y = gpu_solve(P, r, 2, [0], [1])
    ref = r[:, :3].astype(LD) / P[:, :3].astype(LD)
    assert np.all(np.abs(Y.astype(LD) - ref) <= 2.0 ** -52 * np.abs(ref))
    sub = gpu_solve(*precisions(40, 2, 5), 2, [3, 20], [10, 7])                       # runs that cover a part of the rows
    assert np.all(np.isnan(sub[:3])) and np.all(np.isnan(sub[13:20])) and np.all(np.isnan(sub[27:]))
    assert np.all(np.isfinite(sub[3:13])) and np.all(np.isfinite(sub[20:27]))


@pytest.mark.parametrize("span", [1, 2, 8])
def test_no_delta_precision_is_the_quotient(amd, span):
    full = layout(run_lengths(span, 130))
    start, length = R.runs_of(full)
    P, r = precisions(len(full), 17, 50 + span)
    P[:, 17:] = 0.0
    r[:, 17:] = 0.0                                                                   # r^D = sum gamma py^D (..): 0 with it
    Y = gpu_solve(P, r, span, start, length)
    ref = r[:, :17].astype(LD) / P[:, :17].astype(LD)
    err = np.abs(Y[full].astype(LD) - ref[full])
    assert np.all(err <= 2.0 ** -52 * np.abs(ref[full]))                              # 1 ulp
    record_measurement("mlpg_no_delta_%d" % span, err_in_ulp=float((err / (2.0 ** -52 * np.abs(ref[full]))).max()))


def test_bad_sizes_are_error_codes(amd):
    torch, c, d = ctx()
    t = torch.zeros(256, dtype=torch.float64, device=d)
    i = torch.zeros(4, dtype=torch.int64, device=d)
    one = torch.ones(4, dtype=torch.int64, device=d)
    bad = (lambda: c.ceps_delta(None, 1, 1, 1, t), lambda: c.ceps_delta(t, 1, 1, 1, None),
           lambda: c.ceps_delta(t, 0, 1, 1, t), lambda: c.ceps_delta(t, 1, 0, 1, t), lambda: c.ceps_delta(t, 1, 129, 1, t),
           lambda: c.ceps_delta(t, 1, 1, 0, t), lambda: c.ceps_delta(t, 1, 1, 9, t),
           lambda: c.mlpg_solve(None, t, 1, 1, 1, i, one, 1, t, t), lambda: c.mlpg_solve(t, None, 1, 1, 1, i, one, 1, t, t),
           lambda: c.mlpg_solve(t, t, 1, 1, 1, i, one, 1, None, t), lambda: c.mlpg_solve(t, t, 1, 1, 1, i, one, 1, t, None),
           lambda: c.mlpg_solve(t, t, 0, 1, 1, i, one, 1, t, t), lambda: c.mlpg_solve(t, t, 1, 0, 1, i, one, 1, t, t),
           lambda: c.mlpg_solve(t, t, 1, 65, 1, i, one, 1, t, t), lambda: c.mlpg_solve(t, t, 1, 1, 0, i, one, 1, t, t),
           lambda: c.mlpg_solve(t, t, 1, 1, 9, i, one, 1, t, t), lambda: c.mlpg_solve(t, t, 1, 1, 1, i, one, -1, t, t),
           lambda: c.mlpg_solve(t, t, 1, 1, 1, None, one, 1, t, t), lambda: c.mlpg_solve(t, t, 1, 1, 1, i, None, 1, t, t))
    for k, call in enumerate(bad):
        with pytest.raises(RuntimeError, match="error -1"):
            call()
            print("case", k, "returned no error")
    assert c.mlpg_work_len(1, 65, 1) == -1 and c.mlpg_work_len(5, 3, 2) == 90
    Y = torch.full((4, 1), np.nan, dtype=torch.float64, device=d)
    c.mlpg_solve(t, t, 4, 1, 2, None, None, 0, t, Y)                                  # no runs: valid, nothing is written
    assert bool(torch.isnan(Y).all())


# ---- 3. training and conversion end to end
_E2E = {}


def e2e():
    if not _E2E:
        CA, CB, X, Y, M, span = R.dynamic_case()
        _E2E.update(CA=CA, X=X, Y=Y, M=M, span=span, f=R.train(X, Y, M, iters=6, tol=-1.0),
                    g=R.train(X, Y, M, iters=6, tol=-1.0, dtype=LD))
    return _E2E


def model_map(f, span):
    """The model's float64 map as a conversion dict."""
    return dict(weights=f["weights"], means=f["means"], covs=f["covs"], zbar=f["zbar"], phi=f["phi"], loglik=f["loglik"],
                n=np.int64(f["n"]), dx=np.int64(f["dx"]), dy=np.int64(f["dy"]), level=np.bool_(f["level"]), A=f["A"],
                b=f["b"], Wx=np.tril(f["Wx"]), kx=f["kx"], span=np.int64(span), py=f["py"])


def test_dynamic_training_against_the_model(amd):
    import test_gpu_gmm as TG
    e = e2e()
    X, Y, M, span, f, g = (e[k] for k in ("X", "Y", "M", "span", "f", "g"))
    got = amd.dynamic_rows(e["CA"], span)
    keep = ~np.isneginf(e["CA"][:, 0])
    assert np.abs(got[keep] - X).max() <= 2 * (2 * span + 2) * 2.0 ** -53 * 2 * np.abs(e["CA"][keep]).max()
    conv = amd.conversion_train(X, Y, M, span=span, iters=6, tol=0.0)
    assert int(conv["span"]) == span and conv["py"].shape == (M, 8) and int(conv["dx"]) == 8 and int(conv["dy"]) == 8
    assert set(conv) == {"weights", "means", "covs", "zbar", "phi", "loglik", "n", "dx", "dy", "level", "A", "b", "Wx", "kx",
                         "span", "py"}
    N, dx = len(X), 8
    c = np.hstack((R.select(X, 5, False), R.select(Y, 5, False))) - f["zbar"]
    mu_c = f["means"] - f["zbar"]
    W, k = G.estep_parameters(f["weights"], mu_c, f["covs"])
    bar_ll = TG.estep_bars(c, mu_c, W, k)[4]
    gam, ca = f["gamma"], np.abs(c)
    S0 = gam.sum(axis=0)
    floor = dict(loglik=float(bar_ll.mean()), weights=float(2 * (N + 1) * U * S0.max() / N),
                 means=float((2 * (N + 4) * U * (gam.T @ ca) / S0[:, None]).max()),
                 covs=float(max((2 * (N + 4) * U * ((ca * gam[:, m:m + 1]).T @ ca) / S0[m]).max() for m in range(M))))
    floor["py"] = float((f["py"] ** 2).max() * floor["covs"] * (1.0 + np.abs(f["A"]).sum(axis=2).max()) ** 2)
    for key in ("loglik", "weights", "means", "covs", "py"):
        model = float(np.abs(f[key].astype(LD) - g[key]).max())
        err = float(np.abs(conv[key] - f[key]).max())
        bar = max(100.0 * model, floor[key])
        print("dynamic loop %s: |gpu - model| %.3g, model f64 - long double %.3g, floor %.3g" % (key, err, model, floor[key]))
        record_measurement("mlpg_loop_%s" % key, err=err, model_diff=model, one_step_floor=floor[key],
                           err_over_model_diff=err / model if model > 0 else None)
        assert err <= bar, (key, err, bar)
    out = amd.conversion_trajectory(conv, e["CA"])                                    # the trained map converts
    assert out.shape == (len(keep), 5) and np.all(np.isfinite(out[keep]))
    assert np.all(np.isneginf(out[~keep, 0])) and np.all(out[~keep, 1:] == 0.0)
    assert np.array_equal(out[keep, 0], e["CA"][keep, 0])                             # the level: the source's, bit for bit
    with pytest.raises(ValueError, match="conversion_trajectory"):
        amd.conversion_apply(conv, e["CA"])


def test_trajectory_against_the_model(amd):
    import test_gpu_gmm as TG
    e = e2e()
    CA, span, f, g = e["CA"], e["span"], e["f"], e["g"]
    M, dx, dys = e["M"], 8, 4
    out = amd.conversion_trajectory(model_map(f, span), CA)
    t64, tld = R.trajectory(f, CA, span), R.trajectory(f, CA, span, LD)              # the same float64 map in both
    keep = ~np.isneginf(CA[:, 0])
    assert np.array_equal(out[:, 0], CA[:, 0]) and np.all(out[~keep, 1:] == 0.0)
    full, P, r, gamma = R.trajectory_inputs(f, CA, span)
    Xc = R.select(R.dynamic_rows(CA, span)[keep], 5, False) - f["zbar"][:dx]
    mu_c = f["means"] - f["zbar"]
    bar_gamma = TG.estep_bars(Xc, mu_c[:, :dx], np.tril(f["Wx"]), f["kx"])[5]
    bar_r = TG.regress_bar(Xc, gamma, f["py"][:, :, None] * f["A"], f["py"] * (f["b"] + f["zbar"][dx:]))
    e_in = float((bar_gamma.astype(np.float64) / np.maximum(gamma, 1e-300)).clip(max=1.0).max() * M
                 + bar_r.astype(np.float64).max() / np.abs(r).max())
    start, length = R.runs_of(keep)
    rows = np.flatnonzero(keep)
    worst = 0.0
    for s, T in zip(np.concatenate(([0], np.cumsum(length)[:-1])), length):
        idx = rows[s:s + T]
        for d in range(dys):
            Rm, _ = R.system(P[s:s + T], r[s:s + T], span, d)
            floor = float(np.linalg.cond(Rm)) * (2 * c_of(span) * 2.0 ** -53 + e_in) * np.linalg.norm(t64[idx, 1 + d])
            model = np.linalg.norm((t64[idx, 1 + d] - tld[idx, 1 + d]).astype(np.float64))
            err = np.linalg.norm(out[idx, 1 + d] - t64[idx, 1 + d])
            assert err <= max(100.0 * model, floor), (int(s), int(T), d, err, model, floor)
            worst = max(worst, err / max(100.0 * model, floor))
    print("trajectory: |gpu - model| / bar <= %.3g" % worst)
    record_measurement("mlpg_trajectory", err_over_bar=worst, err=float(np.abs(out[keep] - t64[keep]).max()),
                       model_diff=float(np.abs(t64[keep] - tld[keep]).max()))


def test_step_response_through_the_public_function(amd):
    conv, C = R.step_case()
    y = amd.conversion_trajectory(conv, C)
    ref = R.trajectory(conv, C, 1)
    rough, rough_ref = float(np.abs(np.diff(y[:, 1])).max()), float(np.abs(np.diff(ref[:, 1])).max())
    print("step case: largest adjacent difference %.12g (model %.12g)" % (rough, rough_ref))
    record_measurement("mlpg_step_case", roughness=rough, model=rough_ref)
    assert abs(rough - rough_ref) <= 1e-9 and rough < 0.25 and abs(rough_ref - R.STEP_ROUGHNESS) <= 1e-9
    assert np.array_equal(y[:, 0], C[:, 0])
    holed = C.copy()
    holed[100] = (-np.inf, 0.0)                                                       # a gap at the step: nothing couples across it
    z = amd.conversion_trajectory(conv, holed)
    assert np.isneginf(z[100, 0]) and z[100, 1] == 0.0
    assert np.abs(z[:100, 1] + 1.0).max() <= 1e-12 and np.abs(z[101:, 1] - 1.0).max() <= 1e-12
