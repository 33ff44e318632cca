"""The joint-density mixture on the MI355X (convert.gmm_fit / conversion_train / conversion_apply -> eaqhm_gmm_estep,
eaqhm_gmm_mstep, eaqhm_gmm_regress) against the NumPy model of DESIGN.md §12 (tests/gmm_ref.py) in np.longdouble.
Hand-built inputs only.

Bars (u = 2^-53; every bar is TWICE a worst-case rounding bound that holds for any order of summation, computed in long
double from absolute values, plus the allowances for the library functions named below).

E-step.  d_j = c_j - mu_j carries one rounding; y_k = sum_j W_kj d_j is a sum of at most D products in some order:
|dy_k| <= ey_k = (D + 2) u sum_j |W_kj d_j|.  q = sum_k y_k^2: the squares of the perturbed y differ by at most
2 |y_k| ey_k + ey_k^2, and squaring and adding D terms in any order costs (D + 2) u sum_k (|y_k| + ey_k)^2; eq is the
sum of both.  lp = k - q / 2: eq / 2 + u |lp|.  bar_lp = 2 (eq / 2 + u |lp|) + 4 ulp(|lp|) (the issue's allowance for
the library log behind k).  It is checked directly where M = 1 (ll = lp) and enters the other two:
ll = max + ln sum_m exp(lp_m - max) moves by at most max_m |dlp_m| when the lp move (log-sum-exp is 1-Lipschitz in the
sup norm); evaluating it adds, relative to the sum s, 4 ulp for exp, one for the rounding of lp - max (x e^-x < 1) and
(M - 1) u for the additions, then 4 ulp of |ln s| <= ln M for log and u |ll| for the last addition:
bar_ll = max_m bar_lp + 2 (2^-52 (5 + M / 2 + 4 ln M) + u |ll|).
gamma_m = exp(lp_m - max) / s: its relative error is the absolute error of lp_m - ll, at most bar_lp_m + bar_ll, plus
4 ulp for exp and one for the division: bar_gamma = gamma (bar_lp_m + bar_ll + 5 2^-52) + 2^-1070 (the last term: below
2^-1022 a double has fewer bits).  The kernel forms gamma as e / s rather than exp(lp - ll), the same number, so that a
row sums to 1 within M 2^-52 whatever |ll| is; that is asserted too.

M-step.  S2[m][i][j] is a sum of N three-factor products in some order: 2 (N + 4) u sum_n |gamma_nm c_ni c_nj|; S1
likewise with two factors; S0: (N + 1) u S0, as the issue states it (a sum of N exact products gamma x 1 in any order
errs by at most (N - 1) u S0: it needs no factor two).

Regression.  2 (dx + M + 4) u sum_m gamma_nm (|b_m| + sum_j |A_m[:, j] x_j|) per entry.

The loop.  100 x the model's own float64-to-long-double difference per quantity, floored at the one-step bars above
(the model difference can be exactly 0).  Measured ratios (GPU - model float64) / (model float64 - long double) are
recorded; on the MI355X they were at most 2.8 (log-likelihood), 1.1 (weights), 0.9 (means) and 1.0 (covariances), and
the kernels' errors at most 0.042 (ll), 0.052 (gamma), 0.077 (S2), 0.038 (S1), 0.11 (S0) and 0.11 (regression) of their
bars."""
import numpy as np
import pytest

import gmm_ref as R
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


def dev(a):
    torch, c, d = ctx()
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=d)


# ---- the three entry points on host arrays
def gpu_estep(c_rows, mu, W, k):
    torch, c, d = ctx()
    N, D = c_rows.shape
    M = len(k)
    gamma = torch.full((N, M), np.nan, dtype=torch.float64, device=d)
    ll = torch.full((N,), np.nan, dtype=torch.float64, device=d)
    c.gmm_estep(dev(c_rows), N, D, M, dev(mu), dev(W), dev(k), gamma, ll)
    return gamma.cpu().numpy(), ll.cpu().numpy()


def gpu_mstep(c_rows, gamma):
    torch, c, d = ctx()
    N, D = c_rows.shape
    M = gamma.shape[1]
    work = torch.full((c.gmm_work_len(N, D, M),), np.nan, dtype=torch.float64, device=d)
    S0 = torch.full((M,), np.nan, dtype=torch.float64, device=d)
    S1 = torch.full((M, D), np.nan, dtype=torch.float64, device=d)
    S2 = torch.full((M, D, D), np.nan, dtype=torch.float64, device=d)
    c.gmm_mstep(dev(c_rows), dev(gamma), N, D, M, work, S0, S1, S2)
    return S0.cpu().numpy(), S1.cpu().numpy(), S2.cpu().numpy()


def gpu_regress(X, gamma, A, b):
    torch, c, d = ctx()
    N, dx = X.shape
    M, dy = b.shape
    Y = torch.full((N, dy), np.nan, dtype=torch.float64, device=d)
    c.gmm_regress(dev(X), dev(gamma), dev(A), dev(b), N, dx, dy, M, Y)
    return Y.cpu().numpy()


# ---- hand-built problems
SHAPES = [(1, 1, 1), (15, 2, 1), (16, 16, 2), (17, 17, 3), (63, 15, 2), (65, 37, 5), (130, 128, 2), (300, 64, 17),
          (257, 3, 64), (5000, 36, 8)]
_PROBLEMS = {}


def problem(N, D, M):
    """Centred rows c float64[N, D] and the parameters (mu, W, k) of one model M-step (float64, floor 1e-3) on seeded
    clustered data of max(N, 4 M) rows with every label present; computed once per shape and shared."""
    key = (N, D, M)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(10000 * N + 100 * D + M)
        P = max(N, 4 * M)
        labels = rng.permutation(np.arange(P) % M)
        mix = np.eye(D) + rng.standard_normal((D, D)) / np.sqrt(D)
        Z = 3.0 * rng.standard_normal((M, D))[labels] + rng.standard_normal((P, D)) @ mix + 5.0
        zbar, c, phi = R.centre(Z, 1e-3)
        w, mu, Sigma = R.mstep(c, R.one_hot(labels, M), phi)
        W, k = R.estep_parameters(w, mu, Sigma)
        _PROBLEMS[key] = (np.ascontiguousarray(c[:N]), mu, W, k)
    return _PROBLEMS[key]


def estep_bars(c, mu, W, k):
    """(lp, ll, gamma of the long-double model; bar_lp [N, M], bar_ll [N], bar_gamma [N, M]) as the docstring derives."""
    c, mu, W, k = (np.asarray(a, dtype=np.float64).astype(LD) for a in (c, mu, W, k))
    N, D = c.shape
    M = len(k)
    lp, ll, gamma = R.estep(c, mu, np.tril(W), k)
    bar_lp = np.empty((N, M), dtype=LD)
    for m in range(M):
        d = c - mu[m]
        Wm = np.tril(W[m])
        y = d @ Wm.T
        ey = (D + 2) * U * (np.abs(d) @ np.abs(Wm).T)
        eq = (2 * np.abs(y) * ey + ey * ey).sum(axis=1) + (D + 2) * U * ((np.abs(y) + ey) ** 2).sum(axis=1)
        bar_lp[:, m] = 2 * (eq / 2 + U * np.abs(lp[:, m])) + 4 * ULP * np.abs(lp[:, m])
    bar_ll = bar_lp.max(axis=1) + 2 * (ULP * (5 + LD(M) / 2 + 4 * np.log(LD(M))) + U * np.abs(ll))
    bar_gamma = gamma * (bar_lp + bar_ll[:, None] + 5 * ULP) + LD(2.0) ** -1070
    return lp, ll, gamma, bar_lp, bar_ll, bar_gamma


# ---- 1. the E-step
@pytest.mark.parametrize("N,D,M", SHAPES)
def test_estep_against_long_double(amd, N, D, M):
    c, mu, W, k = problem(N, D, M)
    gamma, ll = gpu_estep(c, mu, W, k)
    lp_r, ll_r, gamma_r, bar_lp, bar_ll, bar_gamma = estep_bars(c, mu, W, k)
    e_ll = np.abs(ll.astype(LD) - ll_r)
    e_g = np.abs(gamma.astype(LD) - gamma_r)
    worst_ll, worst_g = float((e_ll / bar_ll).max()), float((e_g / bar_gamma).max())
    print("estep (%d, %d, %d): |dll| / bar <= %.3g, |dgamma| / bar <= %.3g, max |dll| %.3g"
          % (N, D, M, worst_ll, worst_g, float(e_ll.max())))
    record_measurement("gmm_estep_%d_%d_%d" % (N, D, M), ll_err_over_bar=worst_ll, gamma_err_over_bar=worst_g,
                       ll_err=float(e_ll.max()), gamma_err=float(e_g.max()))
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(gamma))
    if M == 1:
        assert np.all(np.abs(ll.astype(LD) - lp_r[:, 0]) <= bar_lp[:, 0])            # ll is lp itself
        assert np.all(gamma == 1.0)
    assert np.all(e_ll <= bar_ll)
    assert np.all(e_g <= bar_gamma)
    assert np.all(np.abs(gamma.sum(axis=1) - 1.0) <= M * 2.0 ** -52)


def test_estep_far_row_and_upper_triangle(amd):
    """A row 40 standard deviations from every mean: every lp is hugely negative, nothing is NaN.  And the entries of W
    above the diagonal are not read: NaN there changes nothing."""
    N, D, M = 65, 37, 5
    c, mu, W, k = problem(N, D, M)
    far = c.copy()
    far[13] = mu[0] + 40.0 * np.linalg.solve(W[0], np.ones(D) / np.sqrt(D))          # ||W_0 (c - mu_0)|| = 40
    gamma, ll = gpu_estep(far, mu, W, k)
    lp_r = R.estep(far.astype(LD), mu.astype(LD), W.astype(LD), k.astype(LD))[0]
    assert float(lp_r[13].max()) < -700.0
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(gamma))
    assert np.all(np.abs(gamma.sum(axis=1) - 1.0) <= M * 2.0 ** -52)
    keep = np.arange(N) != 13
    g0, l0 = gpu_estep(c, mu, W, k)
    assert np.array_equal(gamma[keep], g0[keep]) and np.array_equal(ll[keep], l0[keep])   # rows do not see each other
    Wn = W.copy()
    Wn[:, np.triu_indices(D, 1)[0], np.triu_indices(D, 1)[1]] = np.nan
    g1, l1 = gpu_estep(c, mu, Wn, k)
    assert np.array_equal(g1, g0) and np.array_equal(l1, l0)


def test_estep_row_beyond_the_range(amd):
    """A row so far out that every q overflows to +inf (lp = -inf for every component): ll = -inf and gamma = 1 / M, not
    NaN; the other rows of its block are not touched."""
    c, mu, W, k = problem(17, 17, 3)
    out = c.copy()
    out[5] = 1e200
    gamma, ll = gpu_estep(out, mu, W, k)
    assert ll[5] == -np.inf and np.all(gamma[5] == 1.0 / 3.0)
    keep = np.arange(17) != 5
    g0, l0 = gpu_estep(c, mu, W, k)
    assert np.array_equal(gamma[keep], g0[keep]) and np.array_equal(ll[keep], l0[keep])


# ---- 2. the M-step
def chunk_shapes():
    from eaqhm_amd.convert import gmm_chunk_rows
    R0 = gmm_chunk_rows(1)
    assert all(gmm_chunk_rows(n) == R0 for n in (R0 - 1, R0, R0 + 1, 2 * R0 + 3))
    return [(R0, 5, 3), (R0 - 1, 5, 3), (R0 + 1, 5, 3), (2 * R0 + 3, 5, 3)]


def gammas(N, M, seed):
    """One-hot, dense, and dense with a column of exact zeros (M = 1: the column is the only one)."""
    rng = np.random.default_rng(seed)
    hot = R.one_hot(rng.integers(0, M, size=N), M)
    dense = rng.dirichlet(np.ones(M), size=N)
    holed = dense.copy()
    holed[:, M // 2] = 0.0
    return (("one_hot", hot), ("dense", dense), ("zero_column", holed))


@pytest.mark.parametrize("N,D,M", SHAPES + [(512, 5, 3), (511, 5, 3), (513, 5, 3), (1027, 5, 3)])
def test_mstep_against_long_double(amd, N, D, M):
    assert [s for s in chunk_shapes() if s == (N, D, M)] or (N, D, M) in SHAPES
    c = problem(N, D, M)[0]
    cl, ca = c.astype(LD), np.abs(c)
    worst = worst0 = worst1 = 0.0
    for kind, g in gammas(N, M, N + D + M):
        S0, S1, S2 = gpu_mstep(c, g)
        again = gpu_mstep(c, g)
        for a, b in zip((S0, S1, S2), again):
            assert np.array_equal(a, b), kind                                          # the same bits on every run
        assert np.array_equal(S2, S2.transpose(0, 2, 1)), kind                       # symmetric bit for bit
        gl = g.astype(LD)
        r0, r1 = gl.sum(axis=0), gl.T @ cl
        b0 = (N + 1) * U * r0
        b1 = 2 * (N + 4) * U * (g.T @ ca).astype(LD)
        e0, e1 = np.abs(S0.astype(LD) - r0), np.abs(S1.astype(LD) - r1)
        assert np.all(e0 <= b0) and np.all(e1 <= b1), kind
        worst0 = max(worst0, float((e0[b0 > 0] / b0[b0 > 0]).max()) if np.any(b0 > 0) else 0.0)
        worst1 = max(worst1, float((e1[b1 > 0] / b1[b1 > 0]).max()) if np.any(b1 > 0) else 0.0)
        for m in range(M):
            r2 = (cl * gl[:, m:m + 1]).T @ cl
            b2 = 2 * (N + 4) * U * ((ca * g[:, m:m + 1]).T @ ca).astype(LD)
            e2 = np.abs(S2[m].astype(LD) - r2)
            assert np.all(e2 <= b2), (kind, m)
            if float(b2.max()) > 0:
                worst = max(worst, float((e2[b2 > 0] / b2[b2 > 0]).max()))
        if kind == "zero_column":
            z = M // 2
            assert S0[z] == 0.0 and np.all(S1[z] == 0.0) and np.all(S2[z] == 0.0)
    print("mstep (%d, %d, %d): |dS0| / bar <= %.3g, |dS1| / bar <= %.3g, |dS2| / bar <= %.3g"
          % (N, D, M, worst0, worst1, worst))
    record_measurement("gmm_mstep_%d_%d_%d" % (N, D, M), S0_err_over_bar=worst0, S1_err_over_bar=worst1,
                       S2_err_over_bar=worst)


# ---- 3. the regression
@pytest.mark.parametrize("N,dx,dy,M", [(1, 1, 1, 1), (17, 3, 5, 2), (64, 18, 18, 8), (130, 64, 64, 3),
                                       (1000, 50, 19, 32)])
def test_regress_against_long_double(amd, N, dx, dy, M):
    rng = np.random.default_rng(7 * N + dx + dy + M)
    X = rng.standard_normal((N, dx)) * 2.0
    g = rng.dirichlet(np.ones(M), size=N)
    A = rng.standard_normal((M, dy, dx)) / np.sqrt(dx)
    b = rng.standard_normal((M, dy))
    Y = gpu_regress(X, g, A, b)
    ref = R.regress(X.astype(LD), g.astype(LD), A.astype(LD), b.astype(LD))
    bar = regress_bar(X, g, A, b)
    err = np.abs(Y.astype(LD) - ref)
    worst = float((err / bar).max())
    print("regress (%d, %d, %d, %d): |dY| / bar <= %.3g" % (N, dx, dy, M, worst))
    record_measurement("gmm_regress_%d_%d_%d_%d" % (N, dx, dy, M), err_over_bar=worst, err=float(err.max()))
    assert np.all(err <= bar)


def regress_bar(X, g, A, b):
    M, dy, dx = A.shape
    mag = np.abs(b)[None] + np.einsum("mij,nj->nmi", np.abs(A), np.abs(X))            # [N, M, dy]
    return 2 * (dx + M + 4) * U * np.einsum("nm,nmi->ni", g, mag).astype(LD)


# ---- 4. the loop
_LOOP = {}


def loop_reference(name):
    """(Z, M, d, the model's fit in float64, in long double): 6 rounds, never stopped early; computed once."""
    if name not in _LOOP:
        X, Y, _, M = R.case(name)
        Z = np.hstack((X, Y))
        d = X.shape[1]
        _LOOP[name] = (Z, M, d, R.fit(Z, M, iters=6, tol=-1.0, split=d),
                       R.fit(Z, M, iters=6, tol=-1.0, split=d, dtype=LD))
    return _LOOP[name]


@pytest.mark.parametrize("name", ["ovl_700x3", "ovl_1500x8", "ovl_257x1"])
def test_loop_against_the_model(amd, name):
    Z, M, d, f, g = loop_reference(name)
    N, D = Z.shape
    fit = amd.gmm_fit(Z, M, iters=6, tol=0.0, split=d)
    assert len(fit["loglik"]) == 6 and fit["n"] == N
    assert np.diff(fit["loglik"]).min() >= -1e-12
    assert np.array_equal(fit["zbar"], f["zbar"]) and np.array_equal(fit["phi"], f["phi"])
    # the one-step bars with the model's last responsibilities: what a single E or M step may differ by
    c = (Z - f["zbar"])
    mu_c = f["means"] - f["zbar"]
    W, k = R.estep_parameters(f["weights"], mu_c, f["covs"])
    _, _, _, _, bar_ll, _ = estep_bars(c, mu_c, W, k)
    gam, ca = f["gamma"], np.abs(c)
    S0 = gam.sum(axis=0)
    floor = dict(loglik=float(bar_ll.mean()), weights=float(2 * (N + 1) * U * S0.max() / N),
                 means=float((2 * (N + 4) * U * (gam.T @ ca) / S0[:, None]).max()),
                 covs=float(max((2 * (N + 4) * U * ((ca * gam[:, m:m + 1]).T @ ca) / S0[m]).max() for m in range(M))))
    ratios = {}
    for key in ("loglik", "weights", "means", "covs"):
        model = float(np.abs(f[key].astype(LD) - g[key]).max())
        err = float(np.abs(fit[key] - f[key]).max())
        bar = max(100.0 * model, floor[key])
        ratios[key] = err / model if model > 0 else None                               # None: the model's two agree exactly
        print("loop %s %s: |gpu - model| %.3g, model f64 - long double %.3g, floor %.3g" % (name, key, err, model,
                                                                                            floor[key]))
        record_measurement("gmm_loop_%s_%s" % (name, key), err=err, model_diff=model, one_step_floor=floor[key],
                           err_over_model_diff=ratios[key])
        assert err <= bar, (key, err, bar)
    for S in fit["covs"]:
        assert np.array_equal(S, S.T)


def test_early_stop_is_a_prefix(amd):
    Z, M, d = loop_reference("ovl_257x1")[:3]
    full = amd.gmm_fit(Z, M, iters=40, tol=0.0, split=d)["loglik"]
    short = amd.gmm_fit(Z, M, iters=40, tol=1e-5, split=d)["loglik"]
    assert 2 <= len(short) <= len(full) and np.array_equal(short, full[:len(short)])
    if len(short) < 40:
        assert short[-1] - short[-2] < 1e-5
    assert np.all(np.diff(short)[:-1] >= 1e-5)
    gamma, ll = amd.gmm_posteriors(amd.gmm_fit(Z, M, iters=3, tol=0.0, split=d), Z)
    assert gamma.shape == (len(Z), M) and ll.shape == (len(Z),)
    assert np.all(np.abs(gamma.sum(axis=1) - 1.0) <= M * 2.0 ** -52)


# ---- 5. it learns the map
def test_it_learns_the_map(amd):
    X, Y, _, M = R.case("sep_1500x8")
    conv = amd.conversion_train(X, Y, M, level=True)
    out = amd.conversion_apply(conv, X)
    assert out.shape == Y.shape
    rms = float(np.sqrt(np.mean((out - Y) ** 2)))
    Xa = np.hstack((X, np.ones((len(X), 1))))
    lin = float(np.sqrt(np.mean((Xa @ np.linalg.lstsq(Xa, Y, rcond=None)[0] - Y) ** 2)))
    print("conversion: rms %.4g = %.3f sigma = %.4f of the global linear fit's" % (rms, rms / R.SIGMA, rms / lin))
    record_measurement("gmm_conversion_sep_1500x8", rms_over_sigma=rms / R.SIGMA, rms_over_linear=rms / lin)
    assert rms <= 1.25 * R.SIGMA and rms <= 0.1 * lin


# ---- 6. pass-through and layout
def cepstra(n, P, seed):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((n, P + 1)) / (1.0 + np.arange(P + 1))[None, :] ** 1.5
    C[:, 0] = -4.0 + 0.5 * rng.standard_normal(n)
    return C


@pytest.fixture(scope="module")
def cepstral_map(amd):
    """A map between two sets of cepstrum-like rows of order 12 and 10, two components, level left out."""
    CA = cepstra(400, 12, 1)
    CA[:200, 1] += 1.0
    CB = np.hstack((CA[:, :1] + 0.7, 0.8 * CA[:, 1:11] + 0.05 * cepstra(400, 9, 2)))
    return amd.conversion_train(CA, CB, 2), CA


def test_level_and_empty_rows(amd, cepstral_map):
    conv, CA = cepstral_map
    assert int(conv["dx"]) == 12 and int(conv["dy"]) == 10 and not bool(conv["level"])
    C = CA[:70].copy()
    out = amd.conversion_apply(conv, C)
    assert out.shape == (70, 11) and np.array_equal(out[:, 0], C[:, 0])              # the level: the source's, bit for bit
    holed = C.copy()
    for i in (0, 5, 64, 69):
        holed[i] = 0.0
        holed[i, 0] = -np.inf
    out_h = amd.conversion_apply(conv, holed)
    empty = np.isneginf(holed[:, 0])
    assert np.all(np.isneginf(out_h[empty, 0])) and np.all(out_h[empty, 1:] == 0.0)
    assert np.array_equal(out_h[~empty], out[~empty])                                  # the others: not affected


def test_one_component_is_the_linear_regression(amd):
    """M = 1: yhat = mu_y + Sigma_yx Sigma_xx^-1 (x - mu_x), the closed form in long double from the fitted mixture."""
    rng = np.random.default_rng(21)
    X = rng.standard_normal((300, 8)) @ (np.eye(8) + 0.2 * rng.standard_normal((8, 8)))
    Y = X @ rng.standard_normal((8, 8)) / np.sqrt(8.0) + 1.0 + 0.1 * rng.standard_normal((300, 8))
    conv = amd.conversion_train(X, Y, 1, level=True, iters=2)
    out = amd.conversion_apply(conv, X)
    mu, S = conv["means"][0].astype(LD), conv["covs"][0].astype(LD)
    L = R.cholesky(S[:8, :8])
    Wx = R.tri_inverse(L)
    A = S[8:, :8] @ Wx.T @ Wx
    ref = mu[8:] + (X.astype(LD) - mu[:8]) @ A.T
    xc = X - conv["zbar"][:8]
    bar = regress_bar(xc, np.ones((300, 1)), conv["A"], conv["b"]) + 2 * U * np.abs(ref)   # + the zbar_y added back
    err = np.abs(out.astype(LD) - ref)
    worst = float((err / bar).max())
    print("M = 1 against the closed form: |d| / bar <= %.3g" % worst)
    record_measurement("gmm_one_component_linear", err_over_bar=worst, err=float(err.max()))
    assert np.all(err <= bar)


def test_converted_rows_drive_the_synthesis(amd, cepstral_map):
    conv, CA = cepstral_map
    n, fs, step = 40, 16000, 80
    src = CA[:n].copy()
    src[17] = 0.0
    src[17, 0] = -np.inf
    rows = amd.conversion_apply(conv, src)
    f0 = 125.0 + 15.0 * np.sin(np.maximum(np.arange(n) - 5, 0) / 6.0)   # flat at first: no short run among the first instants
    voiced = np.ones(n, bool)
    voiced[30:33] = False
    det = amd.model_from_parameters(f0, src, fs, step, voiced=voiced)
    L = (n - 1) * step + 1
    s = amd.eaQHMSynthesis(det, fs, L, envelope=rows)
    assert s.shape == (L,) and np.all(np.isfinite(s)) and np.abs(s).max() > 0
    env = amd.cepstrum_envelope(rows, fs, np.linspace(0.0, fs / 2, 9))
    assert env.shape == (n, 9) and np.all(np.isneginf(env[17])) and np.all(np.isfinite(env[np.arange(n) != 17]))
    built = amd.model_from_parameters(f0, rows, fs, step, voiced=voiced)
    assert np.all(np.isfinite(amd.eaQHMSynthesis(built, fs, L)))


# ---- 7. failures are exceptions
def starving():
    """Two separated clusters of 20 rows in 2-D and label 1 on a single row of the first: S0_1 = 1 after the first M-step,
    0.99998824 after the next E-step in the model (the cluster's other rows take a little of it back)."""
    rng = np.random.default_rng(5)
    Z = np.vstack((rng.standard_normal((20, 2)), rng.standard_normal((20, 2)) + 8.0))
    init = np.zeros(40, dtype=np.int64)
    init[7] = 1
    return Z, init


def test_starved_component_raises(amd):
    Z, init = starving()
    with pytest.raises(np.linalg.LinAlgError, match="component 1"):
        R.fit(Z, 2, iters=3, tol=0.0, init=init)                                       # the model does
    with pytest.raises(np.linalg.LinAlgError, match="component 1"):
        amd.gmm_fit(Z, 2, iters=3, tol=0.0, init=init)


def test_nan_is_a_value_error_before_any_launch(amd, monkeypatch):
    from eaqhm_amd import functions
    Z = starving()[0].copy()
    Z[3, 1] = np.nan

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)
    with pytest.raises(ValueError):
        amd.gmm_fit(Z, 2)
    with pytest.raises(ValueError):
        amd.conversion_train(Z, Z, 2)


def test_bad_sizes_are_error_codes(amd):
    torch, c, d = ctx()
    t = torch.zeros(64, dtype=torch.float64, device=d)
    for call in (lambda: c.gmm_estep(t, 0, 1, 1, t, t, t, t, t), lambda: c.gmm_estep(t, 1, 129, 1, t, t, t, t, t),
                 lambda: c.gmm_estep(t, 1, 1, 65, t, t, t, t, t), lambda: c.gmm_mstep(t, t, 1, 0, 1, t, t, t, t),
                 lambda: c.gmm_mstep(t, None, 1, 1, 1, t, t, t, t), lambda: c.gmm_regress(t, t, t, t, 1, 65, 1, 1, t),
                 lambda: c.gmm_regress(t, t, t, t, 1, 1, 0, 1, t), lambda: c.gmm_regress(t, t, t, t, -1, 1, 1, 1, t)):
        with pytest.raises(RuntimeError, match="error -1"):
            call()
    assert c.gmm_work_len(1, 1, 65) == -1
