"""NumPy model of the piecewise-linear formant warp, written from the definition and
independently of the HIP kernels; the GPU tests compare the kernels with it.

A warp is a strictly increasing piecewise-linear map W through (0, 0) and the breakpoints (x_j, y_j), j = 0..B-1,
continued past the last one with the last slope.  What is evaluated is its inverse V at an output frequency q:

    b = min(#{j : y_j <= q}, B - 1),    V(q) = x_{b-1} + (q - y_{b-1}) * ((x_b - x_{b-1}) / (y_b - y_{b-1})),

x_{-1} = y_{-1} = 0, in this order of operations; a row y that equals x bit for bit is the identity, V(q) = q.

    warp_inverse(x, y, q, dtype) / warp_forward(x, y, f, dtype)
    rows(y, n) -> [n, B]
    amplitudes(am, fm, fs, beta, x, y) -> A' (float64[No_ti, Kmax])
    envelope_readout(records, freqs, x, y) -> float64[No_ti, len(freqs)]
    synthesize(records, step, fs, L, rho, beta, x, y) -> float64[L_out]      (rho, beta numbers or contours)
    noise_warp(sigma, refl, x, y, dtype) -> (sigma', refl', stop)             (x, y in cycles per sample)
    noise_envelope(sigma, refl, x, y, fnorm, dtype) -> [Nf, len(fnorm)]
    frame_rows(hop, Nf, ti, y) -> [Nf, B]

`dtype` selects the arithmetic (np.float64: the definition; np.longdouble: the yardstick the GPU tests take the noise
bars from, as noise_warp_ref.warp does).  The inputs are float64 values in either case.
"""
import numpy as np

import model_contour_ref as MC
import model_formant_ref as MF
import model_synthesis_ref as M
import noise_model_ref as N
import noise_warp_ref as W


def is_identity(x, y):
    return np.array_equal(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))


def warp_inverse(x, y, q, dtype=np.float64):
    """V(q) for one row y (both [B]); q any shape."""
    q = np.asarray(q, dtype=np.float64).astype(dtype)
    if is_identity(x, y):
        return q.copy()
    x = np.asarray(x, dtype=np.float64).astype(dtype)
    y = np.asarray(y, dtype=np.float64).astype(dtype)
    B = len(x)
    xp = np.concatenate((np.zeros(1, dtype), x[:-1]))        # x_{b-1}, y_{b-1} for b = 0..B-1
    yp = np.concatenate((np.zeros(1, dtype), y[:-1]))
    ratio = (x - xp) / (y - yp)
    b = np.minimum((y <= q[..., None]).sum(axis=-1), B - 1)
    return xp[b] + (q - yp[b]) * ratio[b]


def warp_forward(x, y, f, dtype=np.float64):
    """W(f): the map itself (the tests' round trip V(W(f)) == f)."""
    f = np.asarray(f, dtype=np.float64).astype(dtype)
    x = np.asarray(x, dtype=np.float64).astype(dtype)
    y = np.asarray(y, dtype=np.float64).astype(dtype)
    B = len(x)
    xp = np.concatenate((np.zeros(1, dtype), x[:-1]))
    yp = np.concatenate((np.zeros(1, dtype), y[:-1]))
    b = np.minimum((x <= f[..., None]).sum(axis=-1), B - 1)
    return yp[b] + (f - xp[b]) * ((y - yp) / (x - xp))[b]


def rows(y, n):
    """y [B] or [n, B] as [n, B]."""
    y = np.asarray(y, dtype=np.float64)
    return np.broadcast_to(y, (n, y.shape[-1]))


def amplitudes(am, fm, fs, beta, x, y):
    """A' of §9.4: exp(E_i(V_i(beta_i f))) for an active slot, 0 for an inactive one and where beta_i f >= fs/2; am (a
    copy) at an instant with an identity row and beta_i == 1."""
    n = am.shape[0]
    beta = np.broadcast_to(np.asarray(beta, dtype=np.float64), (n,))
    y = rows(y, n)
    out = np.zeros_like(am)
    for i in range(n):
        if beta[i] == 1.0 and is_identity(x, y[i]):
            out[i] = am[i]
            continue
        ks = np.flatnonzero((am[i] != 0) & (fm[i] > 0))
        if len(ks) == 0:
            continue
        f, v = MF.envelope_nodes(am[i], fm[i])
        bf = beta[i] * fm[i, ks]
        out[i, ks] = np.exp(M.interp_envelope(f, v, warp_inverse(x, y[i], bf)))
        out[i, ks[bf >= fs / 2]] = 0.0
    return out


def envelope_readout(records, freqs, x, y):
    """out[i, t] = E_i(V_i(freqs[t])); -inf on the rows of instants without active slots."""
    rec = np.asarray(records, dtype=np.float64)
    n, K = rec.shape[0], (rec.shape[1] - 1) // 3
    y = rows(y, n)
    freqs = np.asarray(freqs, dtype=np.float64)
    out = np.full((n, len(freqs)), -np.inf)
    for i in range(n):
        f, v = MF.envelope_nodes(rec[i, :K], rec[i, K:2 * K])
        if len(f):
            out[i] = M.interp_envelope(f, v, warp_inverse(x, y[i], freqs))
    return out


def synthesize(records, step, fs, L, rho, beta, x, y):
    """§9 (rho and beta numbers) or §9.1 (either a contour) with the amplitudes of the warp."""
    rec = np.asarray(records, dtype=np.float64)
    n, K = rec.shape[0], (rec.shape[1] - 1) // 3
    Ap = amplitudes(rec[:, :K], rec[:, K:2 * K], fs, beta, x, y)
    with MF._amplitudes(Ap):
        if np.ndim(rho) or np.ndim(beta):
            rho_v = np.broadcast_to(np.asarray(rho, dtype=np.float64), (n,)).copy()
            beta_v = np.broadcast_to(np.asarray(beta, dtype=np.float64), (n,)).copy()
            return MC.synthesize_contour(rec, step, fs, L, rho_v, beta_v, True)
        return M.synthesize(rec, step, fs, L, rho, beta, True)


def _grid_angles(x, y, dt):
    """w_t = min(2 pi V(t / 2M), pi), t = 0..M."""
    return np.minimum((2 * dt(np.pi)) * warp_inverse(x, y, np.arange(W.M + 1) / (2.0 * W.M), dt), dt(np.pi))


def noise_warp_frame(sigma, k, x, y, dt=np.float64):
    """(sigma', k'[p], stop) of one frame: §10.1's steps with the spectrum read at w = min(2 pi V(t / 2M), pi)."""
    k = np.asarray(k)
    if is_identity(x, y):
        return dt(sigma), k.astype(dt), 0
    if not sigma > 0:
        return dt(0), np.zeros(len(k), dt), 0
    p = len(k)
    a = N.stepup(k.astype(dt))
    P = dt(sigma) * dt(sigma) / W.poly_power(a, _grid_angles(x, y, dt))
    sign = np.where(np.arange(p + 1) % 2 == 0, 1, -1).astype(dt)
    r = (P[0] / 2 + (W.lag_cosines(p, dt) * P[1:W.M]).sum(axis=1) + sign * P[W.M] / 2) / W.M
    k2, E, stop = W.levinson(r, p, dt)
    return np.sqrt(E), k2, stop


def noise_warp(sigma, refl, x, y, dt=np.float64):
    """(sigma'[Nf], refl'[Nf, p], stop[Nf]); x [B], y [B] or [Nf, B] in cycles per sample."""
    sigma = np.asarray(sigma, dtype=np.float64)
    refl = np.asarray(refl, dtype=np.float64)
    y = rows(y, len(sigma))
    s2 = np.zeros(len(sigma), dt)
    k2 = np.zeros(refl.shape, dt)
    stop = np.zeros(len(sigma), dtype=np.int64)
    for m in range(len(sigma)):
        s2[m], k2[m], stop[m] = noise_warp_frame(sigma[m], refl[m], x, y[m], dt)
    return s2, k2, stop


def noise_envelope(sigma, refl, x, y, fnorm, dt=np.float64):
    """out[m, t] = 2 ln sigma_m - ln |A_m(e^{jw})|^2 at w = min(2 pi V_m(fnorm_t), pi); -inf rows for silent frames."""
    sigma = np.asarray(sigma, dtype=np.float64)
    refl = np.asarray(refl, dtype=np.float64)
    y = rows(y, len(sigma))
    out = np.full((len(sigma), len(fnorm)), -np.inf, dtype=dt)
    for m in range(len(sigma)):
        if not sigma[m] > 0:
            continue
        w = np.minimum((2 * dt(np.pi)) * warp_inverse(x, y[m], fnorm, dt), dt(np.pi))
        out[m] = 2 * np.log(dt(sigma[m])) - np.log(W.poly_power(N.stepup(refl[m].astype(dt)), w))
    return out


def frame_rows(hop, Nf, ti, y):
    """y per noise frame from y per analysis instant: every column linear at sample m hop over ti, flat outside."""
    y = np.asarray(y, dtype=np.float64)
    return np.stack([W.contour(hop, Nf, ti, col) for col in y.T], axis=1)


def vtln(fs, alpha, knee=0.875):
    """The two-breakpoint VTLN map of the definition: (f_k, alpha f_k), f_k = knee (fs/2) min(1, 1/alpha); (fs/2, fs/2)."""
    fk = knee * (fs / 2) * min(1.0, 1.0 / alpha)
    return np.array([fk, fs / 2]), np.array([alpha * fk, fs / 2])
