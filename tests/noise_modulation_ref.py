"""NumPy model of the pitch-synchronous modulation of the noise: the fundamental phase of a model,
the analysis of the residual's power envelope over it, the output's fundamental, and the modulated synthesis.
Normative for the tests: the kernels eaqhm_noise_modulation_kernel and eaqhm_noise_combine_mod_kernel compute the same
thing from the same bits of input.  `dt` selects the arithmetic (np.float64: the definition; np.longdouble: the
yardstick the GPU tests take their bars from).  H = hop, W = 4H, D = step, n instants, M harmonics.

Records are float64[n, 3K+1] as unpack_model gives them (|a| (K), f in Hz (K), phase (K), a0); slot k is harmonic k+1.

Order of the sums of the analysis (the kernel's): 64 lanes; lane l adds its samples v = l, l + 64, .. in increasing v
(one multiplication and one addition per term); the 64 partial sums are then added by a butterfly, partner l ^ 32, 16,
8, 4, 2, 1.  e^{2 pi i j theta} comes from one cos / sin of 2 pi frac(theta) by repeated complex multiplication, in the
analysis and in the synthesis."""
import numpy as np

import noise_model_ref as N

MAX_HARMONICS = 8
FLOOR = 0.01


def frac(x):
    y = x - np.floor(x)
    return np.where(y >= 1.0, 0.0, y)


def model_f0(rec):
    """§11's fundamental track (a^2-weighted mean of f_k / (k+1), held over instants without an active slot)."""
    rec = np.asarray(rec, dtype=np.float64)
    n, K = rec.shape[0], (rec.shape[1] - 1) // 3
    out, have = np.zeros(n), np.zeros(n, dtype=bool)
    for i in range(n):
        num = den = 0.0
        for k in range(K):
            a, f = rec[i, k], rec[i, K + k]
            if a != 0 and f > 0:
                num += a * a * (f / (k + 1))
                den += a * a
        if den > 0:
            out[i], have[i] = num / den, True
    if not have.any():
        return np.zeros(n)
    first = int(np.flatnonzero(have)[0])
    for i in range(n):
        if not have[i]:
            out[i] = out[i - 1] if i > first else out[first]
    return out


def model_phase(rec, step, fs, f0=None):
    """Theta_i in cycles, [0, 1): frac(ph_{i,0} / 2 pi) at anchored instants (slot 0 active); the others by the f0
    integral forwards from the previous instant, those before the first anchored one backwards from it; from
    Theta_0 = 0 without any."""
    rec = np.asarray(rec, dtype=np.float64)
    n, K = rec.shape[0], (rec.shape[1] - 1) // 3
    f0 = model_f0(rec) if f0 is None else np.asarray(f0, dtype=np.float64)
    anch = [K > 0 and rec[i, 0] != 0 and rec[i, K] > 0 for i in range(n)]
    th = np.zeros(n)
    first = anch.index(True) if any(anch) else 0
    if any(anch):
        th[first] = frac(rec[first, 2 * K] / (2 * np.pi))
    for i in range(first + 1, n):
        if anch[i]:
            th[i] = frac(rec[i, 2 * K] / (2 * np.pi))
        else:
            th[i] = frac(th[i - 1] + (float(step) / fs) * (f0[i - 1] + f0[i]) / 2)
    for i in range(first - 1, -1, -1):
        th[i] = frac(th[i + 1] - (float(step) / fs) * (f0[i] + f0[i + 1]) / 2)
    return th


def voiced_flags(rec):
    rec = np.asarray(rec, dtype=np.float64)
    K = (rec.shape[1] - 1) // 3
    return ((rec[:, :K] != 0) & (rec[:, K:2 * K] > 0)).any(axis=1)


def nearest(x, ti0, D, n):
    return np.clip(np.rint((np.asarray(x, dtype=np.float64) - float(ti0)) / float(D)), 0, n - 1).astype(np.int64)


def phase_at(x, theta, f0, ti0, D, fs, dt=np.float64):
    """Theta(x) = Theta_i + f0_i (x - ti_i) / fs, i the nearest instant."""
    x = np.asarray(x, dtype=np.float64)
    i = nearest(x, ti0, D, len(theta))
    return theta.astype(dt)[i] + f0.astype(dt)[i] * (x - (float(ti0) + i * float(D))).astype(dt) / dt(fs)


def harmonics_of(th, M, dt=np.float64):
    """(cos, sin)[M, ...] of 2 pi j th, j = 1..M: one cos / sin of the reduced phase, then rotations."""
    th = th - np.floor(th)
    ang = dt(2.0 * np.pi) * th
    c1, s1 = np.cos(ang), np.sin(ang)
    cs, sn = [c1], [s1]
    for _ in range(M - 1):
        cj, sj = cs[-1], sn[-1]
        cs.append(cj * c1 - sj * s1)
        sn.append(sj * c1 + cj * s1)
    return np.array(cs), np.array(sn)


def _wave_sum(terms):
    """terms[..., W] summed in the kernel's order."""
    W = terms.shape[-1]
    pad = (-W) % 64
    if pad:
        terms = np.concatenate((terms, np.zeros(terms.shape[:-1] + (pad,), terms.dtype)), axis=-1)
    rows = terms.reshape(terms.shape[:-1] + (-1, 64))              # [.., t, lane]: v = lane + 64 t
    acc = np.zeros(terms.shape[:-1] + (64,), terms.dtype)
    for t in range(rows.shape[-2]):
        acc = acc + rows[..., t, :]
    lane = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ s]
    return acc[..., 0]


def analyse(e, H, M, theta, f0, voiced, ti0, D, fs, dt=np.float64):
    """mod[Nf, 2M]: Re c_1, Im c_1, .., c_j = sum_v u exp(-2 pi i j Theta) / sum_v u over the frame of §10,
    u = (w e)^2.  Zero rows where not P > 0 and where the instant nearest to mH is unvoiced.  c_j does not depend on
    M (the kernel sums all MAX_HARMONICS of them and stores M)."""
    e = np.asarray(e, dtype=np.float64)
    L = len(e)
    W = 4 * H
    Nf = (L - 1) // H + 1
    v = np.arange(W)
    w = (0.5 - 0.5 * np.cos(np.pi * ((2 * v + 1) / float(W)))).astype(dt)
    pad = np.concatenate((np.zeros(2 * H), e, np.zeros(3 * H))).astype(dt)
    theta, f0 = np.asarray(theta, dtype=np.float64), np.asarray(f0, dtype=np.float64)
    mod = np.zeros((Nf, 2 * M), dt)
    for m in range(Nf):
        if not voiced[nearest(m * H, ti0, D, len(theta))]:
            continue
        x = w * pad[m * H: m * H + W]
        u = x * x
        P = _wave_sum(u)
        if not P > 0:
            continue
        cs, sn = harmonics_of(phase_at(m * H - 2 * H + v, theta, f0, ti0, D, fs, dt), M, dt)
        mod[m, 0::2] = _wave_sum(u * cs) / P
        mod[m, 1::2] = -_wave_sum(u * sn) / P         # the kernel subtracts term by term: the same bits
    return mod


def advance(f0, gain, D, fs):
    """§11's S (cycles): S_0 = 0, S_{j+1} = frac(S_j + (g_j - 1)(D / fs)(f0_j + f0_{j+1}) / 2)."""
    S = np.zeros(len(f0))
    for j in range(len(f0) - 1):
        x = S[j] + (gain[j] - 1.0) * (float(D) / fs) * (f0[j] + f0[j + 1]) / 2
        S[j + 1] = x - np.floor(x)
    return S


def fundamental(rec, step, fs, tau, gain, rate, g_last, f0=None):
    """(theta_q, nu_q) at the input positions tau_q.  gain[n-1] = g_j and rate[n] = rho_j per interval (rate[n-1] and
    g_last hold past the last instant).  j = min(floor(tau / D), n-1), r = tau - jD;
    s = S_j + (g_j - 1)(f0_j r + (f0_{j+1} - f0_j) r^2 / (2D)) / fs;  theta = frac(Theta(tau) + s);
    nu = (g_j / rho_j) F(tau) / fs, F the linear interpolation of f0."""
    rec = np.asarray(rec, dtype=np.float64)
    n, D = rec.shape[0], float(step)
    f0 = model_f0(rec) if f0 is None else np.asarray(f0, dtype=np.float64)
    th_i = model_phase(rec, step, fs, f0)
    S = advance(f0, gain, D, fs)
    tau = np.asarray(tau, dtype=np.float64)
    theta, nu = np.empty(len(tau)), np.empty(len(tau))
    for q, t in enumerate(tau):
        j = min(int(np.floor(t / D)), n - 1)
        r = t - j * D
        fa = f0[j]
        fb = f0[j + 1] if j <= n - 2 else f0[n - 1]
        g = gain[j] if j <= n - 2 else g_last
        s = S[j] + (g - 1.0) * (fa * r + (fb - fa) * r * r / (2.0 * D)) / fs
        theta[q] = frac(phase_at(t, th_i, f0, 0.0, D, fs) + s)
        nu[q] = (g / rate[j]) * np.interp(t, np.arange(n) * D, f0) / fs
    return theta, nu


def frame_mod(mod, H, tau, dt=np.float64):
    """c_q[Nq, 2M]: the blend of §10's frame parameters applied to mod."""
    mod = np.asarray(mod)
    Nf = len(mod)
    mu = np.asarray(tau, dtype=np.float64) / H
    m0 = np.minimum(np.floor(mu).astype(np.int64), Nf - 1)
    m1 = np.minimum(m0 + 1, Nf - 1)
    fr = np.minimum(mu - m0, 1.0).astype(dt)
    return (1 - fr)[:, None] * mod.astype(dt)[m0] + fr[:, None] * mod.astype(dt)[m1]


def gain_of(cq, theta_q, nu_q, d, dt=np.float64):
    """g_q at offsets d (= n' - qH) of one frame: sqrt(max(0.01, 1 + 2 sum_j (Re c cos 2 pi j phi - Im c sin 2 pi j phi)))
    with phi = theta_q + nu_q d, the sum in increasing j."""
    M = len(cq) // 2
    cs, sn = harmonics_of(dt(theta_q) + dt(nu_q) * np.asarray(d, dtype=np.float64).astype(dt), M, dt)
    acc = np.zeros(len(d), dt)
    for j in range(M):
        acc = acc + (cq[2 * j] * cs[j] - cq[2 * j + 1] * sn[j])
    return np.sqrt(np.maximum(dt(FLOOR), 1 + 2 * acc))


def frames(sigma, refl, H, tau, L_out, seed, dt=np.float64):
    """y[2H, Nq]: the kept samples of every output frame's lattice (N.synth's, before the cross-fade)."""
    Nq = (L_out - 1) // H + 1
    p = np.shape(refl)[1]
    sg, k = N.frame_parameters(sigma, refl, H, tau, dt)
    b = np.zeros((p + 1, Nq), dt)
    y = np.zeros((2 * H, Nq), dt)
    qH = np.arange(Nq, dtype=np.int64) * H
    for t in range(4 * H):
        f = sg * N.white(seed, qH - 3 * H + t).astype(dt)
        for i in range(p, 0, -1):
            f = f - k[:, i - 1] * b[i - 1]
            b[i] = b[i - 1] + k[:, i - 1] * f
        b[0] = f
        if t >= 2 * H:
            y[t - 2 * H] = f
    return y


def synth_mod(sigma, refl, H, tau, L_out, seed, mod, theta, nu, dt=np.float64, t_lo=0, t_hi=None, y=None):
    """out[L_out] (zeros outside [t_lo, t_hi)): out[n'] = sum_q v[n' - qH + H] g_q(n') y_q[n'] over the at most two
    frames that cover n', in increasing q; each product from the left."""
    t_hi = L_out if t_hi is None else t_hi
    Nq = (L_out - 1) // H + 1
    y = frames(sigma, refl, H, tau, L_out, seed, dt) if y is None else y
    cq = frame_mod(mod, H, tau, dt)
    v = N.synthesis_window(H).astype(dt)
    d = np.arange(2 * H) - H
    out = np.zeros(L_out, dt)
    for q in range(Nq):
        n = q * H + d
        ok = (n >= t_lo) & (n < t_hi) & (n >= 0)
        if ok.any():
            out[n[ok]] += ((v * gain_of(cq[q], theta[q], nu[q], d, dt)) * y[:, q])[ok]
    return out


def output_phase(theta, nu, H, L_out):
    """The output fundamental's phase (cycles) at every output sample from (theta_q, nu_q): frame q = rint(n' / H)
    (clipped), theta_q + nu_q (n' - qH)."""
    n = np.arange(L_out)
    q = np.clip(np.rint(n / float(H)).astype(np.int64), 0, len(theta) - 1)
    return theta[q] + nu[q] * (n - q * H)


def glide_model(fs=16000, seconds=2.0, step=15, f_lo=180.0, f_hi=300.0, amp=0.1):
    """A one-slot model of a fundamental gliding linearly f_lo -> f_hi (inside the `female` range) with
    ph = 2 pi integral f0: (det arrays dict, records, L)."""
    L = int(round(seconds * fs))
    ti = np.arange(0, L, step, dtype=np.int64)
    t = ti / float(fs)
    T = L / float(fs)
    f = f_lo + (f_hi - f_lo) * t / T
    ph = 2 * np.pi * (f_lo * t + (f_hi - f_lo) * t * t / (2 * T))
    det = dict(ti=ti, amplitudes=np.full((len(ti), 1), amp), frange=f[:, None].copy(), pk=ph[:, None].copy(),
               a0=np.zeros(len(ti)))
    rec = np.column_stack((np.full(len(ti), amp), f, ph, np.zeros(len(ti))))
    return det, rec, L


def modulated_residual(rec, step, fs, L, c1, seed, level=0.01):
    """e[n] = g_true(Theta(n)) x white Gaussian noise, g_true^2(theta) = 1 + 2 Re(c1 exp(2 pi i theta))."""
    th = phase_at(np.arange(L), model_phase(rec, step, fs), model_f0(rec), 0.0, step, fs)
    g2 = 1 + 2 * (c1.real * np.cos(2 * np.pi * th) - c1.imag * np.sin(2 * np.pi * th))
    return level * np.sqrt(g2) * np.random.default_rng(seed).normal(size=L)


def analyse_phase(e, H, M, th):
    """`analyse` against a phase given per sample (th[L], cycles), every frame voiced: the re-analysis of a synthesised
    signal against the output's own fundamental."""
    e = np.asarray(e, dtype=np.float64)
    L, W = len(e), 4 * H
    Nf = (L - 1) // H + 1
    v = np.arange(W)
    w = 0.5 - 0.5 * np.cos(np.pi * ((2 * v + 1) / float(W)))
    pad = np.concatenate((np.zeros(2 * H), e, np.zeros(3 * H)))
    thp = np.concatenate((np.zeros(2 * H), th, np.zeros(3 * H)))
    mod = np.zeros((Nf, 2 * M))
    for m in range(Nf):
        x = w * pad[m * H: m * H + W]
        u = x * x
        P = _wave_sum(u)
        if not P > 0:
            continue
        cs, sn = harmonics_of(thp[m * H: m * H + W], M)
        mod[m, 0::2] = _wave_sum(u * cs) / P
        mod[m, 1::2] = -_wave_sum(u * sn) / P
    return mod
