"""NumPy model of resynthesis from an eaQHM model with time scale rho and pitch scale beta (model.eaQHMSynthesis).

Written from the definition in DESIGN.md ("Resynthesis from the model"), independently of the HIP kernels; the GPU
tests compare the kernels with it.  Everything works on the record layout of include/eaqhm_hip.h:
records[i] = |a| (Kmax), f (Kmax), phase (Kmax), a0 at the knot c_i = i * step.

    synthesize(records, step, fs, L, rho=1, beta=1, preserve_envelope=True) -> float64[rint(rho * L)]
"""
import numpy as np
from scipy.interpolate import make_interp_spline


def run_codes(active):
    """Run codes of eaqhm_spline_solve: 0 inactive, 1 isolated, 2 run of >= 4 knots, 16 + 4*m + pos for runs of
    m = 2 or 3 knots.  Also returns, per slot, the list of runs (first, last)."""
    n, K = active.shape
    code = np.zeros((n, K), dtype=np.uint8)
    runs = []
    for k in range(K):
        a = np.concatenate(([False], active[:, k], [False])).astype(np.int8)
        d = np.diff(a)
        starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1
        runs.append(list(zip(starts.tolist(), ends.tolist())))
        for s, e in runs[-1]:
            m = e - s + 1
            if m == 1:
                code[s, k] = 1
            elif m >= 4:
                code[s:e + 1, k] = 2
            else:
                code[s:e + 1, k] = 16 + 4 * m + np.arange(m)
    return code, runs


def envelope_amplitudes(am, fm, fs, beta, preserve_envelope):
    """A' (step 2 of the definition): exp of the piecewise-linear log-amplitude envelope of each instant, sampled at
    beta * f; muted at or above Nyquist.  beta == 1 returns am unchanged."""
    if beta == 1.0:
        return am.copy()
    out = np.zeros_like(am)
    for i in range(am.shape[0]):
        ks = np.flatnonzero((am[i] != 0) & (fm[i] > 0))
        if len(ks) == 0:
            continue
        q = beta * fm[i, ks]
        if not preserve_envelope:
            out[i, ks] = am[i, ks]
        else:
            order = np.lexsort((ks, fm[i, ks]))           # nodes sorted by (f, k)
            f = fm[i, ks][order]
            v = np.log(am[i, ks][order])
            out[i, ks] = np.exp(interp_envelope(f, v, q))
        out[i, ks[q >= fs / 2]] = 0.0
    return out


def interp_envelope(f, v, q):
    """E(q) on sorted nodes (f, v): flat outside [f[0], f[-1]], the first tied node at a node's own frequency,
    linear between the last node below q and the first node above it."""
    n = len(f)
    idx = np.searchsorted(f, q, side="left")                  # first node with f >= q
    out = np.empty(len(q))
    for t, (j, x) in enumerate(zip(idx, q)):
        if j < n and f[j] == x:
            out[t] = v[j]
        elif j == 0:
            out[t] = v[0]
        elif j == n:
            out[t] = v[n - 1]
        else:
            out[t] = v[j - 1] + (v[j] - v[j - 1]) * ((x - f[j - 1]) / (f[j] - f[j - 1]))
    return out


def _fm_piece_values(fm_col, active_col, s, e, D):
    """fm of the run [s, e] at the samples c_s .. c_e (interp1d kind=3 / the padded short-run cubic)."""
    m = e - s + 1
    knots = np.arange(s, e + 1) * D
    if m >= 4:
        x, y = knots, fm_col[s:e + 1]
    else:
        npad = 4 - m
        pad = np.arange(npad)
        x = np.concatenate((pad * D, knots))
        y = np.concatenate((np.where(active_col[pad], fm_col[pad], 0.0), fm_col[s:e + 1]))
    return make_interp_spline(x.astype(np.float64), y, k=3)(np.arange(knots[0], knots[-1] + 1, dtype=np.float64))


def knot_phases(rec, step, fs):
    """Per slot: code, runs, and for every in-run interval j the local phase sums
    loc[j, u] = sum_{v=1..u} w_j(v) - sum_{v=0..u} sin(pi v/D) er_j (u = 0..D), the unwrapped knot phase R (step 1)
    and the phase of each run's first knot."""
    n = rec.shape[0]
    K = (rec.shape[1] - 1) // 3
    am, fm, ph = rec[:, :K], rec[:, K:2 * K], rec[:, 2 * K:3 * K]
    D = int(step)
    active = am != 0
    code, runs = run_codes(active)
    scale = 2.0 * np.pi / fs
    ft = np.sin(np.pi * np.arange(D + 1) / D)
    S = np.cumsum(ft)[-1]
    loc = {}
    R = np.zeros((n, K))
    ph0 = np.zeros((n, K))
    for k in range(K):
        tab = np.zeros((n - 1, D + 1))
        for s, e in runs[k]:
            if e == s:
                continue
            dense = _fm_piece_values(fm[:, k], active[:, k], s, e, D)
            nint = e - s
            idx = np.arange(nint)[:, None] * D + np.arange(D + 1)[None, :]
            acc = np.cumsum(scale * dense[idx], axis=1)           # the eval kernel's summation order
            w0 = acc[:, 0]
            shift = ph[s:e, k] - w0
            err = (acc[:, -1] + shift) - ph[s + 1:e + 1, k]
            Mr = np.rint(err / (2.0 * np.pi))
            er = np.pi * (err - 2.0 * np.pi * Mr) / (2.0 * D)
            er[-1] = (err[-1] - 2.0 * np.pi * Mr[-1]) / S      # a run's last interval closes its mismatch fully
            c = np.cumsum(ft[None, :] * er[:, None], axis=1)
            tab[s:e] = (acc - w0[:, None]) - c
            delta = (ph[s + 1:e + 1, k] - ph[s:e, k]) + 2.0 * np.pi * Mr
            R[s + 1:e + 1, k] = np.cumsum(delta)
            ph0[s:e + 1, k] = ph[s, k]
        loc[k] = tab
    return code, runs, loc, R, ph0


def synthesize(records, step, fs, L, rho=1.0, beta=1.0, preserve_envelope=True):
    rec = np.asarray(records, dtype=np.float64)
    n = rec.shape[0]
    K = (rec.shape[1] - 1) // 3
    D = int(step)
    am, fm, ph, a0c = rec[:, :K], rec[:, K:2 * K], rec[:, 2 * K:3 * K], rec[:, 3 * K]
    code, runs, loc, R, ph0 = knot_phases(rec, D, fs)
    Ap = envelope_amplitudes(am, fm, fs, beta, preserve_envelope)
    Lp = int(np.rint(rho * L))
    npr = np.arange(Lp, dtype=np.float64)
    tau = npr / rho
    j = np.floor(tau / D).astype(np.int64)
    r = tau - j * float(D)
    lo = r < 0
    j[lo] -= 1
    hi = r >= D
    j[hi] += 1
    r = tau - j * float(D)
    br = beta * rho
    synth = np.zeros(Lp)
    for k in range(K):
        inrun = (code[:-1, k] != 0) & (code[1:, k] != 0)             # interval j of slot k
        jk = j.copy()
        rk = r.copy()
        ok = (jk >= 0) & (jk <= n - 2)
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
            psi0 = R[jj, k] + tab[jj, u0]
            psi1 = R[jj, k] + tab[jj, np.minimum(u0 + 1, D)]
            phi = ph0[jj, k] + br * ((1.0 - fr) * psi0 + fr * psi1)
            A = ((Ap[jj + 1, k] - Ap[jj, k]) / D) * rr + Ap[jj, k]
            cell[cov] = np.where(A != 0, A * np.cos(phi), 0.0)
        iso = np.flatnonzero(code[:, k] == 1)
        if len(iso):
            ns = np.rint(rho * (iso * float(D))).astype(np.int64)
            keep = (ns >= 0) & (ns < Lp)
            np.add.at(cell, ns[keep], Ap[iso[keep], k] * np.cos(ph[iso[keep], k]))
        synth += cell
    a0 = make_interp_spline(np.arange(n) * float(D), a0c, k=3)(tau, extrapolate=True)
    return a0 + 2.0 * synth


def records_from_cells(n, K, cells, am, fm, pk, a0):
    """Records from the sparse cell list of a golden fixture (det_cells, det_am, ...)."""
    rec = np.zeros((n, 3 * K + 1))
    i, k = cells[:, 0], cells[:, 1]
    rec[i, k] = am
    rec[i, K + k] = fm
    rec[i, 2 * K + k] = pk
    rec[:, 3 * K] = a0
    return rec
