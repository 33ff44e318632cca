"""NumPy model of the noise model to and from cepstral rows.  Normative for the tests: the kernels
eaqhm_noise_cepstrum_kernel and eaqhm_noise_from_cepstrum_kernel compute the same thing from the same bits of input.
`dt` selects the arithmetic (np.float64: the definition; np.longdouble: the yardstick the GPU tests take their bars
from).

    cepstrum(sigma, refl, Q, dt) -> [Nf, Q + 1]         the LPC-to-cepstrum recursion, c_0 = ln sigma, c_q = h_q / 2
    closed_form(poles, Q) -> [Q]                        c_q = Re sum_i z_i^q / (2 q), q = 1..Q
    grid_spectrum(row, dt) -> [M + 1]                   P[t] = exp(4 sum_q c_q cos(q pi t / M)) by Clenshaw's recurrence
    autocorrelation(P, p, dt) -> [p + 1]                the lag sums of §10.1 on that grid
    levinson(r, p, dt) -> (k, E, stop)                  noise_warp_ref's recursion and stop rule, r[0] not inflated
    from_cepstrum(ceps, p, dt) -> (sigma, refl, stop)   per row: grid spectrum, lag sums, Levinson, sigma = exp(c_0) sqrt(E)
    readout(ceps, w, dt) -> [n, len(w)]                 C(w) = c_0 + 2 sum_q c_q cos(q w), the direct sum
    stepdown(a) -> k                                    reflection coefficients of A(z) = [1, a_1, .., a_p]
    pole_frames(Nf, p, r, seed, silent) -> (sigma, refl, poles)   the synthetic fixtures
"""
import numpy as np

import noise_model_ref as N
import noise_warp_ref as W

M = W.M


def _pi(dt):
    """pi in `dt` (np.pi is only a float64)."""
    return dt(np.pi) if dt is np.float64 else np.arctan(dt(1)) * 4


def cepstrum_frame(sigma, k, Q, dt=np.float64):
    """One row: h_n = -a_n - (sum_{k=max(1,n-p)}^{n-1} (k h_k) a_{n-k}) / n, a_n = 0 past p; (-inf, 0, .., 0) when sigma is
    not > 0."""
    row = np.zeros(Q + 1, dt)
    if not sigma > 0:
        row[0] = -np.inf
        return row
    p = len(k)
    a = np.zeros(max(p, Q) + 1, dt)
    a[:p + 1] = N.stepup(np.asarray(k).astype(dt))
    h = np.zeros(Q + 1, dt)
    for n in range(1, Q + 1):
        kk = np.arange(max(1, n - p), n)
        s = ((kk.astype(dt) * h[kk]) * a[n - kk]).sum() if len(kk) else dt(0)
        h[n] = -a[n] - s / dt(n)
    row[1:] = h[1:] / 2
    row[0] = np.log(dt(sigma))
    return row


def cepstrum(sigma, refl, Q, dt=np.float64):
    sigma = np.asarray(sigma, dtype=np.float64)
    refl = np.asarray(refl, dtype=np.float64)
    return np.stack([cepstrum_frame(sigma[m], refl[m], Q, dt) for m in range(len(sigma))])


def closed_form(poles, Q):
    """c_q = Re sum_i z_i^q / (2 q), q = 1..Q, of 1 / A(z) with the zeros z_i of A (longdouble powers)."""
    z = np.asarray(poles).astype(np.clongdouble)
    q = np.arange(1, Q + 1)
    return np.array([(z ** int(n)).sum().real / (2 * int(n)) for n in q], dtype=np.longdouble)


def grid_spectrum(row, dt=np.float64):
    """P[t] = exp(2 (C(w_t) - c_0)), w_t = pi t / M, t = 0..M: b_q = c_q + (2 cos w b_{q+1} - b_{q+2}), the sum is
    cos w b_1 - b_2; c_0 is not read."""
    c = np.asarray(row).astype(dt)
    cw2 = 2 * np.cos(_pi(dt) * np.arange(M + 1).astype(dt) / M)
    b1 = np.zeros(M + 1, dt)
    b2 = np.zeros(M + 1, dt)
    for q in range(len(c) - 1, 0, -1):
        b1, b2 = c[q] + (cw2 * b1 - b2), b1
    return np.exp(4 * (cw2 * b1 / 2 - b2))


def autocorrelation(P, p, dt=np.float64):
    """r[l] = (P[0] / 2 + sum_{t=1}^{M-1} P[t] cos(pi l t / M) + (-1)^l P[M] / 2) / M, l = 0..p."""
    sign = np.where(np.arange(p + 1) % 2 == 0, 1, -1).astype(dt)
    return (P[0] / 2 + (W.lag_cosines(p, dt) * P[1:M]).sum(axis=1) + sign * P[M] / 2) / M


def levinson(r, p, dt=np.float64):
    """Levinson-Durbin on r[0..p], r[0] > 0, with noise_warp_ref's stop rule (the first |k_i| >= 1 ends it, k_i.. stay
    0) but r[0] as it is: (k[p], E, stop).  The factor 1 + 1e-9 of the analysis is a white floor at -90 dB; on a frame of
    order 50 it alone moves the round trip's coefficients by 1e-2."""
    r = np.array(r, dtype=dt)
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


def from_cepstrum(ceps, p, dt=np.float64):
    """(sigma[Nf], refl[Nf, p], stop[Nf]); an empty row gives a silent frame."""
    C = np.asarray(ceps)
    sigma = np.zeros(len(C), dt)
    refl = np.zeros((len(C), p), dt)
    stop = np.zeros(len(C), dtype=np.int64)
    for m, row in enumerate(C):
        if np.isneginf(row[0]):
            continue
        k, E, stop[m] = levinson(autocorrelation(grid_spectrum(row, dt), p, dt), p, dt)
        refl[m] = k
        sigma[m] = np.exp(row[0].astype(dt)) * np.sqrt(E)
    return sigma, refl, stop


def readout(ceps, w, dt=np.float64):
    """C_m(w) for the angles w (rad): the direct cosine sum, c_0 added last (-inf stays -inf)."""
    C = np.asarray(ceps).astype(dt)
    w = np.asarray(w).astype(dt)
    q = np.arange(1, C.shape[1]).astype(dt)
    return 2 * (np.cos(np.outer(w, q)) @ C[:, 1:].T).T + C[:, :1]


def stepdown(a):
    """k_1..k_p of A(z) = [1, a_1, .., a_p]: k_i = a^{(i)}_i, a^{(i-1)}_j = (a^{(i)}_j - k_i a^{(i)}_{i-j}) / (1 - k_i^2)."""
    a = np.array(a, dtype=np.float64)
    p = len(a) - 1
    k = np.zeros(p)
    for i in range(p, 0, -1):
        k[i - 1] = a[i]
        a = ((a[:i] - k[i - 1] * a[i:0:-1]) / (1 - k[i - 1] ** 2)) if i > 1 else a[:1]
    return k


def pole_frames(Nf, p, r, seed=0, silent=()):
    """Nf all-pole frames of order p from p // 2 conjugate pole pairs (one real pole more when p is odd): moduli uniform
    in [0.5 r, r]; angles in [0.1, 3.0], pair i uniform in the i-th of p // 2 equal parts of that range (resonances
    spread over the band, as formants are: with all angles drawn from the whole range the pairs of an order-63 frame
    pile up, its spectrum spans more than the 16 digits an autocorrelation in float64 carries, and Levinson-Durbin
    breaks down in any arithmetic at hand); stepped down to reflection coefficients; sigma log-uniform in [1e-3, 1e-1],
    0 on the frames listed in `silent`.  Returns (sigma[Nf], refl[Nf, p], poles[Nf, p])."""
    rng = np.random.default_rng([seed, Nf, p, int(round(1000 * r))])
    sigma = 10.0 ** rng.uniform(-3, -1, Nf)
    refl = np.zeros((Nf, p))
    poles = np.zeros((Nf, p), dtype=np.complex128)
    for m in range(Nf):
        n = p // 2
        z = rng.uniform(0.5 * r, r, n) * np.exp(1j * (0.1 + 2.9 * (np.arange(n) + rng.uniform(0, 1, n)) / max(n, 1)))
        z = np.concatenate((z, z.conj()))
        if p % 2:
            z = np.concatenate((z, [rng.uniform(0.5 * r, r) * rng.choice([-1.0, 1.0])]))
        poles[m] = z
        refl[m] = stepdown(np.poly(z).real)
    assert np.abs(refl).max() < 1
    sigma[list(silent)] = 0.0
    return sigma, refl, poles


def noise_model(sigma, refl, hop=80, fs=16000.0):
    """The dict layout of eaQHMNoiseAnalysis around (sigma, refl)."""
    return dict(sigma=np.array(sigma), refl=np.array(refl), hop=hop, order=np.shape(refl)[1], fs=float(fs),
                length=(len(sigma) - 1) * hop + 1)
