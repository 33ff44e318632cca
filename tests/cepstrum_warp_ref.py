"""NumPy model of the discrete cepstrum on an all-pass warped frequency axis, written from the
definition and independently of the HIP kernels and of the host code; the tests compare both with it.  It is built on
the model of the linear axis (tests/model_cepstrum_ref.py, tests/model_build_ref.py) by import.

The warp is taken in its atan2 form,
    Omega_a(w) = w + 2 atan2(a sin w, 1 - a cos w),    |a| <= 0.9,
and never through the rational map of the kernels, so that the two forms check each other.  A warped row c_0..c_P
describes C(w) = c_0 + 2 sum_p c_p cos(p Omega_a(w)) and Phi(w) = -2 sum_p c_p sin(p Omega_a(w)); the fit is
model_cepstrum_ref's with the nodes at Omega_a(w_n); a readout forms the read frequency in Hz (q, q / alpha or
W^-1(q)), holds it to [0, fs/2], and warps it.

    omega(a, w) -> Omega_a(w), in the dtype of w
    rational(a, w) -> (cos, sin) of Omega_a(w) as the rational map of cos w, sin w (the identity the kernels rest on)
    nodes(am_row, fm_row, fs, a, dtype) -> (Omega_a(w_n), v_n)
    system(w, v, P, lam, dtype) -> (G, b)                         model_cepstrum_ref's, on warped nodes
    fit(records, fs, P, lam, a, dtype) -> [No_ti, P + 1]
    series(ceps, fs, f, a, dtype) -> (C, Phi), each [n, F]         direct sums at the held f, c_0 added last
    readout(ceps, fs, q, a, dtype), phase(ceps, fs, q, a, dtype)
    envelope(ceps, fs, freqs, a, alpha=None, warp=None, dtype), envelope_phase(...)   with the read frequency
    amplitudes(am, fm, fs, beta, ceps, a, alpha=None, warp=None)
    build(f0, voiced, ceps, fs, step, a, ...) -> model_build_ref.build's dict, the series taken on the warped axis
    rewarp_matrix(b, P_in, P_out, dtype) -> A [P_out + 1, P_in + 1]   by Oppenheim & Johnson's recursion
    rewarp_quadrature(b, P_in, P_out, N=2**14) -> the same by the midpoint rule on N points, in np.longdouble
    compose(a_in, a_out) -> b = (a_out - a_in) / (1 - a_in a_out)

`dtype` selects the arithmetic (np.float64: the definition; np.longdouble: the yardstick the GPU tests take their bars
from).  The inputs are float64 values in either case.
"""
import contextlib

import numpy as np

import model_build_ref as MB
import model_cepstrum_ref as CR

_pi = CR._pi


def omega(a, w):
    w = np.asarray(w)
    a = w.dtype.type(a)
    return w + 2 * np.arctan2(a * np.sin(w), 1 - a * np.cos(w))


def rational(a, w):
    """(cos Omega_a(w), sin Omega_a(w)) = (((1 + a^2) cos w - 2 a) / d, (1 - a^2) sin w / d), d = 1 + a^2 - 2 a cos w."""
    w = np.asarray(w)
    a = w.dtype.type(a)
    d = 1 + a * a - 2 * a * np.cos(w)
    return ((1 + a * a) * np.cos(w) - 2 * a) / d, (1 - a * a) * np.sin(w) / d


def nodes(am_row, fm_row, fs, a, dtype=np.float64):
    w, v = CR.nodes(am_row, fm_row, fs, dtype)
    return omega(a, w), v


system = CR.system


def fit(records, fs, P, lam, a, dtype=np.float64):
    rec = np.asarray(records, dtype=np.float64)
    n, K = rec.shape[0], (rec.shape[1] - 1) // 3
    out = np.zeros((n, P + 1), dtype=dtype)
    for i in range(n):
        w, v = nodes(rec[i, :K], rec[i, K:2 * K], fs, a, dtype)
        out[i] = CR._solve(*system(w, v, P, lam, dtype)) if len(w) else CR._empty_row(P, dtype)
    return out


def series(ceps, fs, f, a, dtype=np.float64):
    """(C, Phi) at min(max(f, 0), fs/2), f [F] or [n, F]: the direct sums over p, in `dtype`."""
    C = np.asarray(ceps, dtype=np.float64)
    n, P = C.shape[0], C.shape[1] - 1
    x = np.minimum(np.maximum(np.asarray(f, dtype=np.float64), 0.0), fs / 2)
    x = np.broadcast_to(x, (n, np.shape(f)[-1])).astype(dtype)
    Cd = C.astype(dtype)
    th = omega(a, ((2 * _pi(dtype)) * x) / dtype(fs))
    sc, ss = np.zeros(x.shape, dtype=dtype), np.zeros(x.shape, dtype=dtype)
    for p in range(1, P + 1):
        sc += Cd[:, p, None] * np.cos(p * th)
        ss += Cd[:, p, None] * np.sin(p * th)
    with np.errstate(invalid="ignore"):
        return 2 * sc + Cd[:, 0, None], -2 * ss


def readout(ceps, fs, q, a, dtype=np.float64):
    return series(ceps, fs, q, a, dtype)[0]


def phase(ceps, fs, q, a, dtype=np.float64):
    C = np.asarray(ceps, dtype=np.float64)
    return series(np.where(np.isfinite(C), C, 0.0), fs, q, a, dtype)[1]


def envelope(ceps, fs, freqs, a, alpha=None, warp=None, dtype=np.float64):
    with np.errstate(invalid="ignore"):
        return readout(ceps, fs, CR.read_frequency(freqs, np.shape(ceps)[0], alpha, warp), a, dtype)


def envelope_phase(ceps, fs, freqs, a, alpha=None, warp=None, dtype=np.float64):
    return phase(ceps, fs, CR.read_frequency(freqs, np.shape(ceps)[0], alpha, warp), a, dtype)


def amplitudes(am, fm, fs, beta, ceps, a, alpha=None, warp=None):
    """model_cepstrum_ref.amplitudes with the readout on the warped axis."""
    n = am.shape[0]
    bf = np.broadcast_to(np.asarray(beta, dtype=np.float64), (n,))[:, None] * fm
    active = (am != 0) & (fm > 0)
    with np.errstate(invalid="ignore"):
        A = np.exp(readout(ceps, fs, CR.read_frequency(np.where(active, bf, 0.0), n, alpha, warp), a))
    return np.where(active & (bf < fs / 2), A, 0.0)


@contextlib.contextmanager
def _series_on_axis(a):
    """model_build_ref.build reads C and Phi through its module's `series`: this one for the duration."""
    keep = MB.series
    MB.series = lambda ceps, fs, f, dtype=np.float64: series(ceps, fs, f, a, dtype)
    try:
        yield
    finally:
        MB.series = keep


def build(f0, voiced, ceps, fs, step, a, **kw):
    with _series_on_axis(a):
        return MB.build(f0, voiced, ceps, fs, step, **kw)


def compose(a_in, a_out):
    return (a_out - a_in) / (1.0 - a_in * a_out)


def rewarp_matrix(b, P_in, P_out, dtype=np.longdouble):
    """c~ = A c for rows in the layout c_0, c_1, .. of C = c_0 + 2 sum c_p cos(p .): the recursion of Oppenheim &
    Johnson's frequency transformation on the conventional cepstrum k_0 = c_0, k_p = 2 c_p, one input column at a time."""
    b = dtype(b)
    A = np.zeros((P_out + 1, P_in + 1), dtype=dtype)
    for col in range(P_in + 1):
        k = np.zeros(P_in + 1, dtype=dtype)
        k[col] = 1 if col == 0 else 2
        g = np.zeros(P_out + 1, dtype=dtype)
        for i in range(P_in, -1, -1):
            d = g.copy()
            g[0] = k[i] + b * d[0]
            if P_out >= 1:
                g[1] = (1 - b * b) * d[0] + b * d[1]
            for j in range(2, P_out + 1):
                g[j] = d[j - 1] + b * (d[j] - g[j - 1])
        g[1:] /= 2
        A[:, col] = g
    return A


def rewarp_quadrature(b, P_in, P_out, N=2 ** 14):
    """A[p][j] = (1/pi) int_0^pi m_j(Omega_{-b}(x)) cos(p x) dx, m_0 = 1, m_j = 2 cos(j .), by the midpoint rule on N
    points in np.longdouble (the integrand is even, periodic and analytic: the rule converges geometrically)."""
    ld = np.longdouble
    x = (np.arange(N).astype(ld) + ld(0.5)) * _pi(ld) / N
    w = omega(-ld(b), x)
    M = 2 * np.cos(w[:, None] * np.arange(P_in + 1).astype(ld)[None, :])
    M[:, 0] = 1
    return (np.cos(x[:, None] * np.arange(P_out + 1).astype(ld)[None, :]).T @ M) / N


def four_formant_envelope(f, fs, formants=(450.0, 1100.0, 2600.0, 3600.0), bandwidths=(60.0, 80.0, 120.0, 160.0)):
    """ln |1 / A(e^{jw})| of the all-pole filter with these formants (Hz) and bandwidths (Hz), at the frequencies f."""
    z = np.exp(-2j * np.pi * np.asarray(f, dtype=np.float64) / fs)
    A = np.ones(len(z), dtype=complex)
    for F, B in zip(formants, bandwidths):
        r = np.exp(-np.pi * B / fs)
        A *= (1 - r * np.exp(2j * np.pi * F / fs) * z) * (1 - r * np.exp(-2j * np.pi * F / fs) * z)
    return -np.log(np.abs(A))


def noise_from_cepstrum(ceps, p, a, dtype=np.float64):
    """noise_cepstrum_ref.from_cepstrum for rows on the warped axis: P[t] = exp(4 sum_q c_q cos(q Omega_a(pi t / M))) as
    the direct sum, then that model's lag sums and Levinson-Durbin recursion.  (sigma[Nf], refl[Nf, p], stop[Nf])."""
    import noise_cepstrum_ref as NR
    C = np.asarray(ceps, dtype=np.float64)
    sigma, refl = np.zeros(len(C), dtype), np.zeros((len(C), p), dtype)
    stop = np.zeros(len(C), dtype=np.int64)
    th = omega(a, _pi(dtype) * np.arange(NR.M + 1).astype(dtype) / NR.M)
    for m, row in enumerate(C):
        if np.isneginf(row[0]):
            continue
        s = np.zeros(NR.M + 1, dtype)
        for q in range(1, len(row)):
            s += dtype(row[q]) * np.cos(q * th)
        k, E, stop[m] = NR.levinson(NR.autocorrelation(np.exp(4 * s), p, dtype), p, dtype)
        refl[m] = k
        sigma[m] = np.exp(dtype(row[0])) * np.sqrt(E)
    return sigma, refl, stop
