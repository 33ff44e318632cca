"""TEST-ONLY NumPy model of DESIGN.md §12.4, the EM refinement of the mixture sequence of the trajectory conversion, on
top of tests/mlpg_ref.py and tests/gmm_ref.py.  Runnable in float64 and np.longdouble (`dtype=`).

    p(Y_t | X_t) = sum_m pi_tm N(Y_t; E_tm, diag(1 / py_m)),   Y_t(y) = [y_t | (W y)_t],   E_tm = b_m + ybar + A_m X_t
    E:  lp_tm = ln pi_tm + kc_m - 1/2 sum_j py_mj (Y_tj - E_tmj)^2,  ll_t = ln sum_m exp lp_tm,  gamma = exp(lp - ll)
    M:  P = gamma py,  r = sum_m gamma_m py_m E_m,  mlpg_ref.solve

Two rules beyond the formulas: a component whose prior is 0 on a row has gamma exactly 0 there and does not enter the
maximum; a row on which every remaining lp is -inf has ll = -inf and gamma = its prior row.  A quadratic form counts as
overflowed when it exceeds the largest float64, in either precision: the rule is about the device's number format."""
import numpy as np

import gmm_ref as G
import mlpg_ref as R

LD = np.longdouble
F64_MAX = np.finfo(np.float64).max


def constants(py, dtype=np.float64):
    """kc [M] = 1/2 sum_j ln py_mj - (dy / 2) ln 2 pi, dy the columns of py."""
    py = np.asarray(py).astype(dtype)
    two_pi = dtype(8) * np.arctan(dtype(1))
    return np.log(py).sum(axis=1) / 2 - py.shape[1] * np.log(two_pi) / 2


def dynamic_target(Y, span, run_start, run_len, dtype=np.float64):
    """Yd float[n, 2 dy] = [y | delta y], the delta over each run (tau ascending, the index clipped to the run); rows
    outside every run are NaN."""
    Y = np.asarray(Y).astype(dtype)
    n, dy = Y.shape
    Yd = np.full((n, 2 * dy), np.nan, dtype=dtype)
    w = R.window(span, dtype)
    for s, T in zip(run_start, run_len):
        s, T = int(s), int(T)
        y, idx = Y[s:s + T], np.arange(T)
        acc = np.zeros((T, dy), dtype=dtype)
        for tau in range(1, span + 1):
            acc = acc + w[tau - 1] * (y[np.minimum(idx + tau, T - 1)] - y[np.maximum(idx - tau, 0)])
        Yd[s:s + T, :dy], Yd[s:s + T, dy:] = y, acc
    return Yd


def estep(X, prior, A, bq, py, Y, span, run_start, run_len, dtype=np.float64, kc=None):
    """(lp [n, M], ll [n], gamma [n, M]) of the conditional E-step; rows outside every run are NaN.  X [n, dx] centred
    dynamic source rows, prior [n, M], A [M, 2 dy, dx], bq = b + ybar and py [M, 2 dy], Y [n, dy] the static trajectory.
    `kc` [M] replaces constants(py) when given (the numbers a kernel under test was handed)."""
    X, prior, A, bq, py = (np.asarray(a).astype(dtype) for a in (X, prior, A, bq, py))
    n, M = prior.shape
    Yd = dynamic_target(Y, span, run_start, run_len, dtype)
    live = ~np.isnan(Yd[:, 0])
    kc = constants(py, dtype) if kc is None else np.asarray(kc).astype(dtype)
    lp = np.full((n, M), np.nan, dtype=dtype)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        for m in range(M):
            d = Yd[live] - (X[live] @ A[m].T + bq[m])
            q = (py[m] * d * d).sum(axis=1)
            q = np.where(q > F64_MAX, np.inf, q)
            lp[live, m] = np.log(prior[live, m]) + kc[m] - q / 2
        mx = lp[live].max(axis=1)
        lost = np.isneginf(mx)
        safe = np.where(lost, 0, mx)
        e = np.exp(lp[live] - safe[:, None])                          # exp(-inf) = 0: a zero prior gives exactly 0
        ssum = e.sum(axis=1)
        ll_live = np.where(lost, -np.inf, safe + np.log(np.where(lost, 1, ssum)))
        g_live = np.where(lost[:, None], prior[live], e / np.where(lost, 1, ssum)[:, None])
    ll = np.full(n, np.nan, dtype=dtype)
    gamma = np.full((n, M), np.nan, dtype=dtype)
    ll[live], gamma[live] = ll_live, g_live
    return lp, ll, gamma


def inputs(g, C, span, dtype=np.float64):
    """What the loop keeps of a dynamic map `g` (mlpg_ref.train's or a dict of the same fields) and source rows C: dict(full,
    X centred [nf, dx], prior, A, bq, py, start, length) over the non-empty rows, the runs back to back."""
    C = np.asarray(C, dtype=np.float64)
    dx = int(g["dx"])
    full, _, _, prior = R.trajectory_inputs(g, C, span, dtype)
    zbar = np.asarray(g["zbar"]).astype(dtype)
    X = R.select(np.hstack((C.astype(dtype), R.delta_rows(C, span, dtype)))[full], C.shape[1], bool(g["level"])) - zbar[:dx]
    py, A, b = (np.asarray(g[k]).astype(dtype) for k in ("py", "A", "b"))
    _, length = R.runs_of(full)
    start = np.concatenate(([0], np.cumsum(length)[:-1])).astype(np.int64)
    return dict(full=full, X=X, prior=prior, A=A, bq=b + zbar[dx:], py=py, start=start, length=length)


def refine(g, C, span, iters, dtype=np.float64, state=False):
    """conversion_trajectory_em's rows after `iters` refinements: (rows float[n, Q + 1] in model_cepstrum's layout, trace
    float[iters + 1] = sum_t ln p(Y_t(y^(i)) | X_t) for i = 0 .. iters, posteriors float[nf, M] of the last M-step (the
    prior when iters = 0)).  With state=True also dict(P, r, Y, start, length): the last systems and their solution on the
    compacted rows, what the global-variance ascent starts from."""
    C = np.asarray(C, dtype=np.float64)
    skip = 0 if bool(g["level"]) else 1
    dys = int(g["dy"]) // 2
    out = np.zeros((len(C), dys + skip), dtype=dtype)
    k = inputs(g, C, span, dtype)
    full, X, prior, A, bq, py, start, length = (k[f] for f in ("full", "X", "prior", "A", "bq", "py", "start", "length"))
    out[~full, 0] = -np.inf
    pyA, pyb = py[:, :, None] * A, py * bq
    gamma, trace = prior, []
    P, r = gamma @ py, G.regress(X, gamma, pyA, pyb)
    Y = R.solve(P, r, span, start, length, dtype)
    for _ in range(iters):
        _, ll, gamma = estep(X, prior, A, bq, py, Y, span, start, length, dtype)
        trace.append(ll.sum())
        P, r = gamma @ py, G.regress(X, gamma, pyA, pyb)
        Y = R.solve(P, r, span, start, length, dtype)
    trace.append(estep(X, prior, A, bq, py, Y, span, start, length, dtype)[1].sum())
    out[full, skip:] = Y
    if skip:
        out[full, 0] = C[full, 0]
    res = (out, np.array(trace, dtype=dtype), gamma)
    return res + (dict(P=P, r=r, Y=Y, start=start, length=length),) if state else res


def stop_iteration(trace, n, tol, iters):
    """The iterations conversion_trajectory_em(em_tol=tol) does on a trace of totals over n rows: the first i >= 1 whose
    mean rose by less than tol over the one before, else `iters`."""
    mean = np.asarray(trace, dtype=np.float64) / n
    for i in range(1, iters):
        if mean[i] - mean[i - 1] < tol:
            return i
    return iters


def ambiguous_case(T=50, span=1, w0=0.6, p_static=4.0, p_delta=100.0):
    """mlpg_ref.step_case with both x means 0: the source says nothing about the component, the posteriors given X are the
    weights (w0, 1 - w0) on every row, and conversion_trajectory's estimate is the blend w0 - (1 - w0) of the static means
    +1 and -1.  Returns (conv dict, C float64[T, 2])."""
    means = np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, -1.0, 0.0]])
    covs = np.stack([np.diag([1.0, 1e4, 1.0 / p_static, 1.0 / p_delta])] * 2)
    w, zbar = np.array([w0, 1.0 - w0]), np.zeros(4)
    A, b, Wx, kx = G.conversion(w, means - zbar, covs, 2)
    py = np.stack([1.0 / np.diag(covs[m, 2:, 2:] - A[m] @ covs[m, :2, 2:]) for m in range(2)])
    conv = dict(weights=w, means=means, covs=covs, zbar=zbar, phi=np.zeros(4), loglik=np.zeros(1), n=np.int64(T),
                dx=np.int64(2), dy=np.int64(2), level=np.bool_(False), A=A, b=b, Wx=Wx, kx=kx, span=np.int64(span), py=py)
    C = np.zeros((T, 2))
    C[:, 0] = -3.0
    return conv, C


HAND_Y = (0.2, 0.76273937238846, 0.99701967873932, 0.99954202885099)   # y after 0 .. 3 refinements of ambiguous_case()
HAND_LOGLIK = (-25.334614833245, 26.796782228667, 32.362041527236, 32.362680067103)
