"""NumPy model of the formant warp of the noise model: an all-pole frame (sigma, k_1..k_p) is read as
the power spectrum P(w) = sigma^2 / |A(e^{jw})|^2, warped in frequency by alpha on a grid of M + 1 points, turned into
an autocorrelation and re-fitted by the Levinson-Durbin recursion of §10.  Normative for the tests: the kernels
eaqhm_noise_warp_kernel and eaqhm_noise_envelope_kernel compute the same thing from the same bits of input.  `dt`
selects the arithmetic (np.float64: the definition; np.longdouble: the yardstick the GPU tests take their bars from)."""
import numpy as np

import noise_model_ref as N

M = 1024          # grid intervals on [0, pi]; NW_M of csrc/eaqhm_noise.hip


def poly_power(a, w):
    """|A(e^{jw})|^2 for A(z) = sum a_i z^-i at the angles w (1-D): (sum a_i cos(i w))^2 + (sum a_i sin(i w))^2."""
    ang = np.outer(w, np.arange(len(a)).astype(w.dtype))
    re = (np.cos(ang) * a).sum(axis=1)
    im = (np.sin(ang) * a).sum(axis=1)
    return re * re + im * im


_TABLES = {}


def lag_cosines(p, dt=np.float64):
    """c[l, t-1] = cos(pi ((l t) mod 2M) / M), l = 0..p, t = 1..M-1; the reduction of l t is exact in integers."""
    key = (p, np.dtype(dt).name)
    if key not in _TABLES:
        lt = np.outer(np.arange(p + 1, dtype=np.int64), np.arange(1, M, dtype=np.int64)) % (2 * M)
        _TABLES[key] = np.cos(dt(np.pi) * lt.astype(dt) / M)
    return _TABLES[key]


def levinson(r, p, dt=np.float64):
    """Levinson-Durbin as DESIGN.md §10 states it, on r[0..p] with r[0] > 0: (k[p], E, stop)."""
    r = np.array(r, dtype=dt)
    r[0] = r[0] * dt(1 + 1e-9)
    a = np.zeros(p + 1, dt)
    a[0] = 1
    k_out = np.zeros(p, dt)
    E = r[0]
    stop = 0
    for i in range(1, p + 1):
        k = -(r[i] + np.dot(a[1:i], r[i - 1:0:-1])) / E
        if not abs(k) < 1:
            stop = i
            break
        a[1:i] = a[1:i] + k * a[i - 1:0:-1]
        a[i] = k
        E = E * (1 - k * k)
        k_out[i - 1] = k
    return k_out, E, stop


def warped_autocorrelation(sigma, k, alpha, dt=np.float64):
    """r'[0..p] of one frame (sigma > 0, alpha != 1): steps 2 and 3 of the definition."""
    p = len(k)
    a = N.stepup(np.asarray(k).astype(dt))
    t = np.arange(M + 1).astype(dt)
    w = np.minimum(dt(np.pi) * t / M / dt(alpha), dt(np.pi))
    P = dt(sigma) * dt(sigma) / poly_power(a, w)
    sign = np.where(np.arange(p + 1) % 2 == 0, 1, -1).astype(dt)
    return (P[0] / 2 + (lag_cosines(p, dt) * P[1:M]).sum(axis=1) + sign * P[M] / 2) / M


def warp_frame(sigma, k, alpha, dt=np.float64):
    """(sigma', k'[p], stop) of one frame."""
    k = np.asarray(k)
    if alpha == 1.0:
        return dt(sigma), k.astype(dt), 0
    if not sigma > 0:
        return dt(0), np.zeros(len(k), dt), 0
    k2, E, stop = levinson(warped_autocorrelation(sigma, k, alpha, dt), len(k), dt)
    return np.sqrt(E), k2, stop


def warp(sigma, refl, alpha, dt=np.float64):
    """(sigma'[Nf], refl'[Nf, p], stop[Nf]) for alpha a number or one value per frame."""
    sigma = np.asarray(sigma, dtype=np.float64)
    refl = np.asarray(refl, dtype=np.float64)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), sigma.shape)
    s2 = np.zeros(len(sigma), dt)
    k2 = np.zeros(refl.shape, dt)
    stop = np.zeros(len(sigma), dtype=np.int64)
    for m in range(len(sigma)):
        s2[m], k2[m], stop[m] = warp_frame(sigma[m], refl[m], float(alpha[m]), dt)
    return s2, k2, stop


def envelope(sigma, refl, alpha, fnorm, dt=np.float64):
    """out[m, t] = 2 ln sigma_m - ln |A_m(e^{jw})|^2 at w = 2 pi min(fnorm_t / alpha_m, 0.5) (fnorm = f / fs): the
    exact warped log power spectrum of every frame; rows of silent frames are -inf."""
    sigma = np.asarray(sigma, dtype=np.float64)
    refl = np.asarray(refl, dtype=np.float64)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), sigma.shape)
    f = np.asarray(fnorm, dtype=np.float64).astype(dt)
    out = np.full((len(sigma), len(f)), -np.inf, dtype=dt)
    for m in range(len(sigma)):
        if not sigma[m] > 0:
            continue
        w = (2 * dt(np.pi)) * np.minimum(f / dt(alpha[m]), dt(0.5))
        out[m] = 2 * np.log(dt(sigma[m])) - np.log(poly_power(N.stepup(refl[m].astype(dt)), w))
    return out


DB = 10 / np.log(10)       # natural-log power -> dB


def contour(noise_hop, Nf, ti, alpha):
    """alpha per noise frame from alpha per analysis instant: linear at sample m hop over ti, flat outside."""
    return np.interp(np.arange(Nf) * float(noise_hop), np.asarray(ti, dtype=np.float64),
                     np.asarray(alpha, dtype=np.float64))
