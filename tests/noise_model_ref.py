"""NumPy model of the stochastic component: the LPC analysis of a residual and its resynthesis as
filtered white noise.  Normative for the tests: the kernels of csrc/eaqhm_noise.hip compute the same thing from the same
bits of input.  `dt` selects the arithmetic (np.float64: the definition; np.longdouble: the yardstick the GPU tests
take their bars from).  H = hop, p = order, L = signal length."""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
MIX1 = 0xBF58476D1CE4E5B9
MIX2 = 0x94D049BB133111EB


def analysis_window(W):
    """w[v] = 0.5 - 0.5 cos(2 pi (v + 0.5) / W), v = 0..W-1 (float64)."""
    return 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(W) + 0.5) / W)


def synthesis_window(H):
    """v[u] = 0.5 - 0.5 cos(2 pi u / (2H)), u = 0..2H-1 (float64)."""
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(2 * H) / (2 * H))


def analyse(e, H, p, dt=np.float64):
    """(sigma[Nf], refl[Nf, p], stop[Nf]): stop[m] is the stage i at which frame m's recursion stopped (|k_i| >= 1),
    0 if it ran through."""
    e = np.asarray(e, dtype=np.float64).astype(dt)
    L = len(e)
    W = 4 * H
    w = analysis_window(W).astype(dt)
    Nf = (L - 1) // H + 1
    pad = np.concatenate((np.zeros(2 * H, dt), e, np.zeros(3 * H, dt)))
    sigma = np.zeros(Nf, dt)
    refl = np.zeros((Nf, p), dt)
    stop = np.zeros(Nf, dtype=np.int64)
    sw2 = (w * w).sum()
    for m in range(Nf):
        x = w * pad[m * H: m * H + W]
        r = np.array([np.dot(x[l:], x[:W - l]) for l in range(p + 1)], dtype=dt)
        if not r[0] > 0:
            continue
        r[0] = r[0] * dt(1 + 1e-9)
        a = np.zeros(p + 1, dt)
        a[0] = 1
        E = r[0]
        for i in range(1, p + 1):
            k = -(r[i] + np.dot(a[1:i], r[i - 1:0:-1])) / E
            if not abs(k) < 1:
                stop[m] = i
                break
            a[1:i] = a[1:i] + k * a[i - 1:0:-1]
            a[i] = k
            E = E * (1 - k * k)
            refl[m, i - 1] = k
        sigma[m] = np.sqrt(E / sw2)
    return sigma, refl, stop


def white(seed, n):
    """The excitation x[n] for an integer array n: splitmix64 of seed + (n + 1) * GOLDEN, uniform with unit variance;
    0 for n < 0."""
    n = np.asarray(n, dtype=np.int64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.maximum(n, 0).astype(np.uint64) + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        z = z ^ (z >> np.uint64(31))
    x = ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5) * 3.4641016151377544
    return np.where(n >= 0, x, 0.0)


def lattice(k, x):
    """The all-pole lattice of one frame from zero state: per sample f = x[n]; for i = p..1: f -= k_i b[i-1];
    b[i] = b[i-1] + k_i f; b[0] = f; y[n] = f."""
    p = len(k)
    b = np.zeros(p + 1)
    y = np.empty(len(x))
    for n in range(len(x)):
        f = x[n]
        for i in range(p, 0, -1):
            f = f - k[i - 1] * b[i - 1]
            b[i] = b[i - 1] + k[i - 1] * f
        b[0] = f
        y[n] = f
    return y


def stepup(k):
    """A(z) = 1 + sum a_i z^-i of reflection coefficients k_1..k_p: [1, a_1, .., a_p]."""
    a = np.array([1.0])
    for ki in k:
        a = np.concatenate((a, [0.0])) + ki * np.concatenate(([0.0], a[::-1]))
    return a


def frame_parameters(sigma, refl, H, tau, dt=np.float64):
    """sigma_q[Nq] and k_q[Nq, p] of the output frames: linear in mu = tau / H between frames floor(mu) and the next,
    held past the last frame (index and fraction in float64, the blend in dt)."""
    Nf = len(sigma)
    mu = np.asarray(tau, dtype=np.float64) / H
    m0 = np.minimum(np.floor(mu).astype(np.int64), Nf - 1)
    m1 = np.minimum(m0 + 1, Nf - 1)
    fr = np.minimum(mu - m0, 1.0).astype(dt)
    s = np.asarray(sigma).astype(dt)
    k = np.asarray(refl).astype(dt)
    return (1 - fr) * s[m0] + fr * s[m1], (1 - fr)[:, None] * k[m0] + fr[:, None] * k[m1]


def synth(sigma, refl, H, tau, L_out, seed, dt=np.float64):
    """out[L_out]: every output frame q filters the excitation over n' = qH - 3H .. qH + H - 1 from zero state and keeps
    the last 2H samples, windowed by v; frames are added in increasing q.  The lattice runs over all frames at once
    (one vector element per frame); per frame it is `lattice` above."""
    Nq = (L_out - 1) // H + 1
    p = np.shape(refl)[1]
    sg, k = frame_parameters(sigma, refl, H, tau, dt)
    v = synthesis_window(H).astype(dt)
    b = np.zeros((p + 1, Nq), dt)
    y = np.zeros((2 * H, Nq), dt)
    qH = np.arange(Nq, dtype=np.int64) * H
    for t in range(4 * H):
        f = sg * white(seed, qH - 3 * H + t).astype(dt)
        for i in range(p, 0, -1):
            f = f - k[:, i - 1] * b[i - 1]
            b[i] = b[i - 1] + k[:, i - 1] * f
        b[0] = f
        if t >= 2 * H:
            y[t - 2 * H] = f
    out = np.zeros(L_out, dt)
    for q in range(Nq):
        n = q * H - H + np.arange(2 * H)
        ok = (n >= 0) & (n < L_out)
        out[n[ok]] += (v * y[:, q])[ok]
    return out


def time_map(H, L_out, rho):
    """tau_q = (qH) / rho for a time scale rho."""
    return (np.arange((L_out - 1) // H + 1) * float(H)) / rho


def contour_time_map_inverse(H, L_out, C, rate, step):
    """tau_q for the contour map of DESIGN.md §9.1: j = max{j : C_j <= qH}, tau = j step + (qH - C_j) / rate_j (rate_j
    = r_j on the intervals, rho_{n-1} past the last knot)."""
    x = np.arange((L_out - 1) // H + 1) * float(H)
    tau = np.empty(len(x))
    for q, xq in enumerate(x):
        j = max(int(np.flatnonzero(np.asarray(C) <= xq)[-1]), 0)
        tau[q] = j * float(step) + (xq - C[j]) / rate[j]
    return tau


def ar_fixture(seconds=2.0, fs=16000, seed=1):
    """Synthetic AR(4) noise (poles 0.97 e^{+-0.5i}, 0.9 e^{+-2i}) with a gain ramp 0.01 -> 0.05 and a silent stretch
    [0.375, 0.4375) of the length: the fixture of the CPU and GPU tests (fixed generator seed)."""
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    L = int(round(seconds * fs))
    a = np.poly([0.97 * np.exp(0.5j), 0.97 * np.exp(-0.5j), 0.9 * np.exp(2.0j), 0.9 * np.exp(-2.0j)]).real
    e = lfilter([1.0], a, rng.normal(size=L)) * np.linspace(0.01, 0.05, L)
    e[int(0.375 * L):int(0.4375 * L)] = 0.0
    return e


def lpc_log_spectrum(sigma, k, nfft=512):
    """20 log10(sigma / |A(e^{jw})|) on nfft/2 + 1 points."""
    return 20 * np.log10(sigma / np.abs(np.fft.rfft(stepup(k), nfft)))


def stop_stage(sigma, refl):
    """The stage at which a frame's recursion stopped, read off the stored coefficients: the first i with
    k_i .. k_p all exactly zero in a frame that is not silent; 0 if k_p != 0."""
    p = np.shape(refl)[1]
    nz = np.asarray(refl) != 0
    last = np.where(nz.any(axis=1), p - np.argmax(nz[:, ::-1], axis=1), 0)     # index (1-based) of the last nonzero k
    return np.where((np.asarray(sigma) > 0) & (last < p), last + 1, 0)
