"""NumPy model of resynthesis with time and pitch scale contours (model.eaQHMSynthesis with array scales).

Written from the definition in DESIGN.md §9.1, independently of the HIP kernels; the GPU tests compare the contour
kernels with it.  The per-interval pieces (run codes, local phase sums, unwrapped increments, envelope amplitudes) are
those of model_synthesis_ref, which models §9.

    time_map(rho, beta, step, L) -> (rate, gain, C, L_out)
    synthesize_contour(records, step, fs, L, rho, beta, preserve_envelope=True) -> float64[L_out]
"""
import numpy as np
from scipy.interpolate import make_interp_spline

import model_synthesis_ref as M


def time_map(rho, beta, step, L):
    """r_j, g_j per interval, C per knot (float64 cumsum, C_0 = 0) and L_out; rate has rho_{n-1} appended."""
    rho = np.asarray(rho, dtype=np.float64)
    beta = np.asarray(beta, dtype=np.float64)
    n = len(rho)
    r = (rho[:-1] + rho[1:]) / 2
    g = r * ((beta[:-1] + beta[1:]) / 2)
    C = np.concatenate(([0.0], np.cumsum(r * float(step))))
    L_out = int(np.rint(C[-1] + rho[-1] * (L - (n - 1) * step)))
    return np.append(r, rho[-1]), g, C, L_out


def locate(C, rate, D, L_out):
    """Per output sample n': (j, r) of the time map.  j = max{j : C_j <= n'} and r = (n' - C_j) / r_j clamped below D
    while n' < C_{n-1}; past it j = n-1 and r = (n' - C_{n-1}) / rho_{n-1}."""
    n = len(C)
    x = np.arange(L_out, dtype=np.float64)
    past = x >= C[-1]
    j = np.searchsorted(C, x, side="right") - 1
    j = np.minimum(j, n - 2)
    j[past] = n - 1
    r = (x - C[j]) / rate[j]
    inside = ~past
    r[inside] = np.minimum(r[inside], np.nextafter(float(D), 0.0))
    return j, r


def envelope_amplitudes_per_instant(am, fm, fs, beta, preserve_envelope):
    """A'_i: §9's rule applied to every instant with its own beta_i."""
    out = np.empty_like(am)
    for v in np.unique(beta):
        rows = np.flatnonzero(beta == v)
        out[rows] = M.envelope_amplitudes(am[rows], fm[rows], fs, float(v), preserve_envelope)
    return out


def weighted_phases(rec, step, fs, gain):
    """Per slot: code, local phase tables and the weighted knot phase G (0 at a run's first knot,
    G_{j+1} = G_j + g_j Delta_j) with the run's first-knot phase ph0."""
    n = rec.shape[0]
    K = (rec.shape[1] - 1) // 3
    ph = rec[:, 2 * K:3 * K]
    code, runs, loc, R, ph0 = M.knot_phases(rec, step, fs)
    G = np.zeros((n, K))
    for k in range(K):
        for s, e in runs[k]:
            if e == s:
                continue
            dph = ph[s + 1:e + 1, k] - ph[s:e, k]
            # the whole turns M_j, recovered exactly from R's increments
            turns = np.rint(((R[s + 1:e + 1, k] - R[s:e, k]) - dph) / (2.0 * np.pi))
            delta = dph + 2.0 * np.pi * turns
            G[s + 1:e + 1, k] = np.cumsum(gain[s:e] * delta)
    return code, loc, G, ph0


def synthesize_contour(records, step, fs, L, rho, beta, preserve_envelope=True):
    rec = np.asarray(records, dtype=np.float64)
    n = rec.shape[0]
    K = (rec.shape[1] - 1) // 3
    D = int(step)
    am, fm, ph, a0c = rec[:, :K], rec[:, K:2 * K], rec[:, 2 * K:3 * K], rec[:, 3 * K]
    rho = np.asarray(rho, dtype=np.float64)
    beta = np.asarray(beta, dtype=np.float64)
    rate, gain, C, Lp = time_map(rho, beta, D, L)
    code, loc, G, ph0 = weighted_phases(rec, D, fs, gain)
    Ap = envelope_amplitudes_per_instant(am, fm, fs, beta, preserve_envelope)
    j, r = locate(C, rate, D, Lp)
    synth = np.zeros(Lp)
    for k in range(K):
        inrun = (code[:-1, k] != 0) & (code[1:, k] != 0)             # interval j of slot k
        jk = j.copy()
        rk = r.copy()
        ok = jk <= n - 2
        ok[ok] = inrun[jk[ok]]
        last = (~ok) & (rk == 0) & (jk - 1 >= 0) & (jk - 1 <= n - 2)
        last[last] = inrun[jk[last] - 1]
        jk[last] -= 1
        rk[last] = D
        cov = ok | last
        cell = np.zeros(Lp)
        if cov.any():
            jj, rr = jk[cov], rk[cov]
            u0 = np.floor(rr).astype(np.int64)
            fr = rr - u0
            tab = loc[k]
            psi0 = tab[jj, u0]
            psi1 = tab[jj, np.minimum(u0 + 1, D)]
            phi = ph0[jj, k] + G[jj, k] + gain[jj] * ((1.0 - fr) * psi0 + fr * psi1)
            A = ((Ap[jj + 1, k] - Ap[jj, k]) / D) * rr + Ap[jj, k]
            cell[cov] = np.where(A != 0, A * np.cos(phi), 0.0)
        iso = np.flatnonzero(code[:, k] == 1)
        if len(iso):
            ns = np.rint(C[iso]).astype(np.int64)
            keep = (ns >= 0) & (ns < Lp)
            np.add.at(cell, ns[keep], Ap[iso[keep], k] * np.cos(ph[iso[keep], k]))
        synth += cell
    tau = j * float(D) + r
    a0 = make_interp_spline(np.arange(n) * float(D), a0c, k=3)(tau, extrapolate=True)
    return a0 + 2.0 * synth
