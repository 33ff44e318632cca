"""NumPy model of the discrete-cepstrum envelope, written from the definition and independently of
the HIP kernels; the GPU tests compare the kernels with it.

The nodes of an instant are its active slots (am != 0, f > 0) in slot order: w_n = 2 pi f_n / fs, v_n = ln am_n.  With
order P the basis is m_0(w) = 1, m_p(w) = 2 cos(p w), the envelope C(w) = sum_p c_p m_p(w), and the fit

    c = argmin sum_n (v_n - C(w_n))^2 + lam sum_p 8 pi^2 p^2 c_p^2,    (M^T M + lam R) c = M^T v,  R = diag(8 pi^2 p^2).

An instant without nodes gives (-inf, 0, .., 0).

    nodes(am_row, fm_row, fs, dtype) -> (w, v)
    system(w, v, P, lam, dtype) -> (G, b)                      the normal equations
    fit(records, fs, P, lam, dtype) -> [No_ti, P + 1]          the normal equations solved in `dtype`
    fit_qr(records, fs, P, lam) -> float64[No_ti, P + 1]       the augmented system [M; sqrt(lam R)] by QR, refined
    readout(ceps, fs, q, dtype) -> [n, len(q)]                 the direct cosine sum at min(max(q, 0), fs/2)
    clenshaw(ceps, fs, q, dtype) -> [n, len(q)]                the same by Clenshaw's recurrence from one cos
    read_frequency(q, alpha=None, warp=None) -> q, q / alpha or V(q)
    envelope(ceps, fs, freqs, alpha=None, warp=None, dtype) -> [n, F]
    amplitudes(am, fm, fs, beta, ceps, alpha=None, warp=None, dtype) -> A' ([No_ti, Kmax])

`dtype` selects the arithmetic (np.float64: the definition; np.longdouble: the yardstick the GPU tests take their bars
from).  The inputs are float64 values in either case, and so is the held read frequency, as in cepstrum_warp_ref: the
series is what `dtype` computes.  `warp` is (x [B], y [B] or [n, B]) in Hz.
"""
import numpy as np

import formant_warp_ref as FW


def nodes(am_row, fm_row, fs, dtype=np.float64):
    ks = np.flatnonzero((am_row != 0) & (fm_row > 0))
    f = fm_row[ks].astype(dtype)
    return (2 * _pi(dtype)) * f / dtype(fs), np.log(am_row[ks].astype(dtype))


def _pi(dtype):
    """pi in `dtype` (np.pi is only a float64)."""
    return dtype(np.pi) if dtype is np.float64 else np.arctan(dtype(1)) * 4


def penalty(P, dtype=np.float64):
    p = np.arange(P + 1).astype(dtype)
    return 8 * _pi(dtype) ** 2 * p * p


def basis(w, P):
    """M[n][p]: 1, then 2 cos(p w_n)."""
    p = np.arange(P + 1).astype(w.dtype)
    M = 2 * np.cos(w[:, None] * p[None, :])
    M[:, 0] = 1
    return M


def system(w, v, P, lam, dtype=np.float64):
    M = basis(w, P)
    G = M.T @ M + np.diag(dtype(lam) * penalty(P, dtype))
    return G, M.T @ v


def _solve(G, b):
    """Gaussian elimination with partial pivoting in the dtype of G (np.linalg has no long double)."""
    if G.dtype == np.float64:
        return np.linalg.solve(G, b)
    A = np.concatenate((G, b[:, None]), axis=1).copy()
    n = len(b)
    for j in range(n):
        piv = j + int(np.argmax(np.abs(A[j:, j])))
        if piv != j:
            A[[j, piv]] = A[[piv, j]]
        A[j + 1:] -= (A[j + 1:, j] / A[j, j])[:, None] * A[j][None, :]
    x = np.zeros(n, dtype=G.dtype)
    for j in range(n - 1, -1, -1):
        x[j] = (A[j, n] - A[j, j + 1:n] @ x[j + 1:]) / A[j, j]
    return x


def _empty_row(P, dtype):
    row = np.zeros(P + 1, dtype=dtype)
    row[0] = -np.inf
    return row


def fit(records, fs, P, lam, dtype=np.float64):
    rec = np.asarray(records, dtype=np.float64)
    n, K = rec.shape[0], (rec.shape[1] - 1) // 3
    out = np.zeros((n, P + 1), dtype=dtype)
    for i in range(n):
        w, v = nodes(rec[i, :K], rec[i, K:2 * K], fs, dtype)
        out[i] = _solve(*system(w, v, P, lam, dtype)) if len(w) else _empty_row(P, dtype)
    return out


def fit_qr(records, fs, P, lam):
    """The same minimiser without forming M^T M: least squares on [M; sqrt(lam R)] c = [v; 0] by QR in float64, then
    two steps of refinement with the residual of the normal equations taken in np.longdouble."""
    rec = np.asarray(records, dtype=np.float64)
    n, K = rec.shape[0], (rec.shape[1] - 1) // 3
    out = np.zeros((n, P + 1))
    ld = np.longdouble
    for i in range(n):
        w, v = nodes(rec[i, :K], rec[i, K:2 * K], fs)
        if not len(w):
            out[i] = _empty_row(P, np.float64)
            continue
        A = np.concatenate((basis(w, P), np.diag(np.sqrt(lam * penalty(P)))), axis=0)
        rhs = np.concatenate((v, np.zeros(P + 1)))
        Q, Rf = np.linalg.qr(A)
        c = np.linalg.solve(Rf, Q.T @ rhs)
        wl, vl = nodes(rec[i, :K], rec[i, K:2 * K], fs, ld)
        Gl, bl = system(wl, vl, P, lam, ld)
        for _ in range(2):      # (A^T A) dc = b - G c, through the same R factor
            res = (bl - Gl @ c.astype(ld)).astype(np.float64)
            c = c + np.linalg.solve(Rf, np.linalg.solve(Rf.T, res))
        out[i] = c
    return out


def _held(q, fs):
    return np.minimum(np.maximum(np.asarray(q, dtype=np.float64), 0.0), fs / 2)


def readout(ceps, fs, q, dtype=np.float64):
    """C_i(q) = c_0 + 2 sum_p c_p cos(2 pi p q^ / fs) as the direct sum; q is [F] or [n, F].  c_0 is added last."""
    C = np.asarray(ceps, dtype=np.float64).astype(dtype)
    n, P = C.shape[0], C.shape[1] - 1
    x = np.broadcast_to(_held(q, fs), (n, np.shape(q)[-1])).astype(dtype)
    theta = 2 * _pi(dtype) * x / dtype(fs)
    s = np.zeros(x.shape, dtype=dtype)
    for p in range(1, P + 1):
        s += C[:, p, None] * np.cos(p * theta)
    return 2 * s + C[:, 0, None]


def clenshaw(ceps, fs, q, dtype=np.float64):
    """The same by Clenshaw's recurrence from cos(theta) alone: b_p = c_p + 2 cos(theta) b_{p+1} - b_{p+2},
    sum = b_1 cos(theta) - b_2."""
    C = np.asarray(ceps, dtype=np.float64).astype(dtype)
    n, P = C.shape[0], C.shape[1] - 1
    x = np.broadcast_to(_held(q, fs), (n, np.shape(q)[-1])).astype(dtype)
    cw2 = 2 * np.cos(2 * _pi(dtype) * x / dtype(fs))
    b1, b2 = np.zeros(x.shape, dtype=dtype), np.zeros(x.shape, dtype=dtype)
    for p in range(P, 0, -1):
        b1, b2 = C[:, p, None] + (cw2 * b1 - b2), b1
    return 2 * (0.5 * cw2 * b1 - b2) + C[:, 0, None]


def read_frequency(q, n, alpha=None, warp=None):
    """[n, F]: q, q / alpha_i or V_i(q)."""
    q = np.broadcast_to(np.asarray(q, dtype=np.float64), (n, np.shape(q)[-1]))
    if alpha is not None:
        return q / np.broadcast_to(np.asarray(alpha, dtype=np.float64), (n,))[:, None]
    if warp is not None:
        x, y = warp
        y = FW.rows(y, n)
        return np.stack([FW.warp_inverse(x, y[i], q[i]) for i in range(n)])
    return q.copy()


def envelope(ceps, fs, freqs, alpha=None, warp=None, dtype=np.float64):
    n = np.shape(ceps)[0]
    with np.errstate(invalid="ignore"):
        return readout(ceps, fs, read_frequency(freqs, n, alpha, warp), dtype)


def amplitudes(am, fm, fs, beta, ceps, alpha=None, warp=None, dtype=np.float64):
    """A'[i][k] = exp(C_i(read_i(beta_i f_k))) for an active slot, 0 for an inactive one and where beta_i f_k >= fs/2.
    No unit rule."""
    n = am.shape[0]
    bf = np.broadcast_to(np.asarray(beta, dtype=np.float64), (n,))[:, None] * fm
    active = (am != 0) & (fm > 0)
    with np.errstate(invalid="ignore"):
        A = np.exp(readout(ceps, fs, read_frequency(np.where(active, bf, 0.0), n, alpha, warp), dtype))
    return np.where(active & (bf < fs / 2), A, dtype(0))
