"""NumPy model of the shape-invariant phase mode (model.eaQHMSynthesis with phase="shape").

Written from the definition in DESIGN.md §11, independently of the HIP kernels; the GPU tests compare the shape kernels
with it.  The per-interval pieces (run codes, local phase sums Psi, unwrapped knot phases R, envelope amplitudes, time
maps) are those of model_synthesis_ref (§9) and model_contour_ref (§9.1).

    model_f0(records) -> float64[n]
    advance(f0, gain, step, fs) -> S float64[n]
    synthesize_shape(records, step, fs, L, rho, beta, preserve_envelope=True, f0=None, alpha=None, phases=False)
        -> float64[L_out], or (signal, dict(phase=[L_out, K], cover=[L_out, K] bool, tau=[L_out]))
    model_phases(records, step, fs, tau) -> (phase[len(tau), K], cover[len(tau), K]): the model's own phases at tau

rho, beta: numbers (the scalar path: tau = n'/rho, g = beta rho) or arrays of one value per instant (the contour path).
`mode="independent"` gives the phases of §9 / §9.1 through the same code, for tests that tell the modes apart."""
import numpy as np
from scipy.interpolate import make_interp_spline

import model_contour_ref as MC
import model_formant_ref as MF
import model_synthesis_ref as M


def model_f0(records):
    rec = np.asarray(records, dtype=np.float64)
    n = rec.shape[0]
    K = (rec.shape[1] - 1) // 3
    out = np.zeros(n)
    have = np.zeros(n, dtype=bool)
    for i in range(n):
        num = den = 0.0
        for k in range(K):
            a, f = rec[i, k], rec[i, K + k]
            if a != 0 and f > 0:
                num += a * a * f / (k + 1)
                den += a * a
        if den > 0:
            out[i], have[i] = num / den, True
    if not have.any():
        return np.zeros(n)
    for i in range(n):
        if not have[i]:
            earlier = np.flatnonzero(have[:i])
            out[i] = out[earlier[-1]] if len(earlier) else out[np.flatnonzero(have)[0]]
    return out


def advance(f0, gain, step, fs):
    """S_0 = 0; S_{j+1} = frac(S_j + (g_j - 1) (D / fs) (f0_j + f0_{j+1}) / 2), sequentially in float64."""
    S = np.zeros(len(f0))
    for j in range(len(f0) - 1):
        x = S[j] + (gain[j] - 1.0) * (float(step) / fs) * (f0[j] + f0[j + 1]) / 2
        S[j + 1] = x - np.floor(x)
    return S


def _locate_scalar(rho, D, Lp):
    tau = np.arange(Lp, dtype=np.float64) / rho
    j = np.floor(tau / D).astype(np.int64)
    r = tau - j * float(D)
    j[r < 0] -= 1
    j[r >= D] += 1
    r = tau - j * float(D)
    return j, r, tau


def _slot_cover(code, k, j, r, n, D):
    """(cov, jj, rr): the samples slot k has a phase at, their in-run interval and offset (a run's last knot is the
    end rr = D of its last interval)."""
    inrun = (code[:-1, k] != 0) & (code[1:, k] != 0)
    jk, rk = j.copy(), r.copy()
    ok = (jk >= 0) & (jk <= n - 2)
    ok[ok] = inrun[jk[ok]]
    last = (~ok) & (rk == 0) & (jk - 1 >= 0) & (jk - 1 <= n - 2)
    last[last] = inrun[jk[last] - 1]
    jk[last] -= 1
    rk[last] = D
    cov = ok | last
    return cov, jk[cov], rk[cov]


def _psi(tab, Rk, jj, rr, D):
    u0 = np.floor(rr).astype(np.int64)
    fr = rr - u0
    return Rk[jj], (1.0 - fr) * tab[jj, u0] + fr * tab[jj, np.minimum(u0 + 1, D)], fr, u0


def model_phases(records, step, fs, tau):
    """The model's own phase of every slot at the positions tau (samples of the analysed signal): ph_a + R_j + the
    interpolated Psi_j, as §9 has it at rho = beta = 1."""
    rec = np.asarray(records, dtype=np.float64)
    n = rec.shape[0]
    K = (rec.shape[1] - 1) // 3
    D = int(step)
    code, runs, loc, R, ph0 = M.knot_phases(rec, D, fs)
    tau = np.asarray(tau, dtype=np.float64)
    j = np.floor(tau / D).astype(np.int64)
    r = tau - j * float(D)
    j[r < 0] -= 1
    j[r >= D] += 1
    r = tau - j * float(D)
    phase = np.zeros((len(tau), K))
    cover = np.zeros((len(tau), K), dtype=bool)
    for k in range(K):
        cov, jj, rr = _slot_cover(code, k, j, r, n, D)
        if cov.any():
            Rj, loc_i, _, _ = _psi(loc[k], R[:, k], jj, rr, D)
            phase[cov, k] = ph0[jj, k] + (Rj + loc_i)
            cover[cov, k] = True
    return phase, cover


def synthesize_shape(records, step, fs, L, rho=1.0, beta=1.0, preserve_envelope=True, f0=None, alpha=None,
                     phases=False, mode="shape"):
    rec = np.asarray(records, dtype=np.float64)
    n = rec.shape[0]
    K = (rec.shape[1] - 1) // 3
    D = int(step)
    am, fm, ph, a0c = rec[:, :K], rec[:, K:2 * K], rec[:, 2 * K:3 * K], rec[:, 3 * K]
    contour = np.ndim(rho) > 0 or np.ndim(beta) > 0 or np.ndim(alpha) > 0
    code, runs, loc, R, ph0 = M.knot_phases(rec, D, fs)
    if contour:
        rho_v, beta_v = np.broadcast_to(rho, (n,)).astype(np.float64), np.broadcast_to(beta, (n,)).astype(np.float64)
        rate, gain, C, Lp = MC.time_map(rho_v, beta_v, D, L)
        j, r = MC.locate(C, rate, D, Lp)
        tau = j * float(D) + r
        g_last = rho_v[-1] * beta_v[-1]
    else:
        rho_v, beta_v = np.full(n, float(rho)), np.full(n, float(beta))
        Lp = int(np.rint(rho * L))
        j, r, tau = _locate_scalar(float(rho), D, Lp)
        gain = np.full(n - 1, float(beta) * float(rho))
        C = None
        g_last = float(beta) * float(rho)
    if alpha is None:
        if contour:
            Ap = MC.envelope_amplitudes_per_instant(am, fm, fs, beta_v, preserve_envelope)
        else:
            Ap = M.envelope_amplitudes(am, fm, fs, float(beta), preserve_envelope)
    else:
        Ap = MF.formant_amplitudes(am, fm, fs, beta_v, np.broadcast_to(alpha, (n,)).astype(np.float64))
    f0 = model_f0(rec) if f0 is None else np.broadcast_to(np.asarray(f0, dtype=np.float64), (n,))
    S = advance(f0, gain, D, fs)
    # s(n'): interval j of the sample, f0 linear inside it; past the last knot f0 and the rate are held
    jc = np.minimum(j, n - 2)
    inside = j <= n - 2
    fa = np.where(inside, f0[jc], f0[n - 1])
    fb = np.where(inside, f0[jc + 1], f0[n - 1])
    gm1 = np.where(inside, gain[jc], g_last) - 1.0
    s = S[np.minimum(j, n - 1)] + gm1 * (fa * r + (fb - fa) * r * r / (2.0 * D)) / fs
    if mode == "independent" and contour:
        _, _, G, _ = MC.weighted_phases(rec, D, fs, gain)
    synth = np.zeros(Lp)
    phase_out = np.zeros((Lp, K)) if phases else None
    cover_out = np.zeros((Lp, K), dtype=bool) if phases else None
    for k in range(K):
        cov, jj, rr = _slot_cover(code, k, j, r, n, D)
        cell = np.zeros(Lp)
        if cov.any():
            Rj, loc_i, _, _ = _psi(loc[k], R[:, k], jj, rr, D)
            if mode == "shape":
                phi = ph0[jj, k] + (Rj + loc_i) + (2.0 * np.pi * (k + 1)) * s[cov]
            elif contour:
                phi = ph0[jj, k] + G[jj, k] + gain[jj] * loc_i
            else:
                phi = ph0[jj, k] + gain[0] * (Rj + loc_i)
            A = ((Ap[jj + 1, k] - Ap[jj, k]) / D) * rr + Ap[jj, k]
            cell[cov] = np.where(A != 0, A * np.cos(phi), 0.0)
            if phases:
                phase_out[cov, k] = phi
                cover_out[cov, k] = True
        iso = np.flatnonzero(code[:, k] == 1)
        if len(iso):
            ns = np.rint(C[iso] if contour else float(rho) * (iso * float(D))).astype(np.int64)
            keep = (ns >= 0) & (ns < Lp)
            np.add.at(cell, ns[keep], Ap[iso[keep], k] * np.cos(ph[iso[keep], k]))
        synth += cell
    a0 = make_interp_spline(np.arange(n) * float(D), a0c, k=3)(tau, extrapolate=True)
    out = a0 + 2.0 * synth
    if phases:
        return out, dict(phase=phase_out, cover=cover_out, tau=tau, s=s)
    return out


def constructed_model(fs=16000, seconds=2.0, step=15, K=20, f0=140.0):
    """A det_format="arrays" model with a known shape: f0 constant, theta_k(t) = 0.9 sin(2 pi 1.3 t + 0.7 k),
    ph = (k+1) 2 pi f0 t + theta_k, f = (k+1) f0 + theta_k' / 2 pi, a = 1 / (k+1), a0 = 0.  Returns (det, L, closed)
    with closed(rho, beta) -> (expected float64[N], N): 2 sum_k a_k cos(2 pi (k+1) beta f0 n' / fs +
    theta_k(n' / (rho fs))) on the output samples n' < N whose tau does not pass the last knot."""
    L = int(round(seconds * fs))
    ti = np.arange(0, L, step, dtype=np.int64)
    t = ti[:, None] / float(fs)
    k = np.arange(K)[None, :]
    theta = 0.9 * np.sin(2 * np.pi * 1.3 * t + 0.7 * k)
    dtheta = 0.9 * 2 * np.pi * 1.3 * np.cos(2 * np.pi * 1.3 * t + 0.7 * k)
    det = dict(ti=ti, amplitudes=np.broadcast_to(1.0 / (k + 1), theta.shape).copy(),
               frange=(k + 1) * f0 + dtheta / (2 * np.pi), pk=(k + 1) * 2 * np.pi * f0 * t + theta,
               a0=np.zeros(len(ti)))

    def closed(rho, beta):
        N = int(np.floor(rho * float(ti[-1]))) + 1
        npr = np.arange(N, dtype=np.float64)[:, None]
        th = 0.9 * np.sin(2 * np.pi * 1.3 * (npr / (rho * fs)) + 0.7 * k)
        return 2.0 * ((1.0 / (k + 1)) * np.cos(2 * np.pi * (k + 1) * beta * f0 * npr / fs + th)).sum(axis=1), N

    return det, L, closed
