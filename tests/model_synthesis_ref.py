"""NumPy model of resynthesis from an eaQHM model with time scale rho and pitch scale beta (model.eaQHMSynthesis).

Written from the definition in DESIGN.md ("Resynthesis from the model"), independently of the HIP kernels; the GPU
tests compare the kernels with it.  Everything works on the record layout of include/eaqhm_hip.h:
records[i] = |a| (Kmax), f (Kmax), phase (Kmax), a0 at the knot c_i = i * step.

    synthesize(records, step, fs, L, rho=1, beta=1, preserve_envelope=True, dtype=np.float64) -> dtype[rint(rho * L)]

synthesize, knot_phases and envelope_amplitudes take dtype=np.float64 (the definition) or np.longdouble (the yardstick
the direct GPU tests take their bars from).  The long-double path is built from the dtype-generic splines of
interp_stage_ref; what decides a path (run codes, the sample's interval and offset, the read frequency of the
envelope, the muting) is formed in float64 in both, so the two differ by rounding alone.
"""
import numpy as np
from scipy.interpolate import make_interp_spline

import interp_stage_ref as S


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


def envelope_amplitudes(am, fm, fs, beta, preserve_envelope, dtype=np.float64):
    """A' (step 2 of the definition): exp of the piecewise-linear log-amplitude envelope of each instant, sampled at
    beta * f; muted at or above Nyquist.  beta == 1 returns am unchanged.  The read frequency beta * f, which decides
    the node, the node hit and the muting, is formed in float64 whatever `dtype` the envelope is evaluated in."""
    dt = dtype
    if beta == 1.0:
        return am.astype(dt)
    out = np.zeros(am.shape, dt)
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
            v = np.log(am[i, ks][order].astype(dt))
            out[i, ks] = np.exp(interp_envelope(f, v, q, dt))
        out[i, ks[q >= fs / 2]] = 0.0
    return out


def interp_envelope(f, v, q, dtype=np.float64):
    """E(q) on sorted nodes (f, v): flat outside [f[0], f[-1]], the first tied node at a node's own frequency,
    linear between the last node below q and the first node above it."""
    n = len(f)
    idx = np.searchsorted(f, q, side="left")                  # first node with f >= q
    dt = dtype
    out = np.empty(len(q), dt)
    for t, (j, x) in enumerate(zip(idx, q)):
        if j < n and f[j] == x:
            out[t] = v[j]
        elif j == 0:
            out[t] = v[0]
        elif j == n:
            out[t] = v[n - 1]
        else:
            out[t] = v[j - 1] + (v[j] - v[j - 1]) * ((dt(x) - dt(f[j - 1])) / (dt(f[j]) - dt(f[j - 1])))
    return out


def lagrange3(px, py, x, dt):
    """The parabola through three points (interp_stage_ref.lagrange4's sibling)."""
    return _lagrange(px, py, x, dt, 3)


def lagrange2(px, py, x, dt):
    """The line through two points."""
    return _lagrange(px, py, x, dt, 2)


def _lagrange(px, py, x, dt, nn):
    px = np.asarray(px).astype(dt)
    py = np.asarray(py).astype(dt)
    x = np.asarray(x).astype(dt)
    assert len(px) == len(py) == nn
    out = np.zeros(len(x), dt)
    for p in range(nn):
        w = py[p]
        t = np.ones(len(x), dt)
        for q in range(nn):
            if q != p:
                w = w / (px[p] - px[q])
                t = t * (x - px[q])
        out = out + w * t
    return out


def short_run_nodes(fm_col, active_col, s, e, D):
    """Nodes (instants, values) of the fm piece of a run [s, e] of m < 4 knots: the run's own knots and
    those pad instants p in 0 .. 3-m that are not knots of the run; a pad instant carries fm if it is active, else 0."""
    m = e - s + 1
    pad = np.array([p for p in range(4 - m) if not s <= p <= e], dtype=np.int64)
    inst = np.concatenate((pad, np.arange(s, e + 1)))
    y = np.concatenate((np.where(active_col[pad], fm_col[pad], 0.0), fm_col[s:e + 1]))
    return inst, y


def _fm_piece_values(fm_col, active_col, s, e, D, dtype=np.float64):
    """fm of the run [s, e] at the samples c_s .. c_e (interp1d kind=3 / the padded short-run cubic; the polynomial
    of lowest degree through the nodes where pad instants coincide with the run's knots)."""
    dt = dtype
    m = e - s + 1
    knots = np.arange(s, e + 1) * D
    xs = np.arange(knots[0], knots[-1] + 1)
    if m >= 4:
        if dt is np.float64:
            return make_interp_spline(knots.astype(np.float64), fm_col[s:e + 1], k=3)(xs.astype(np.float64))
        y = fm_col[s:e + 1].astype(dt)
        Mo = S.notaknot_moments(y, D, dt)
        j = np.minimum((xs - knots[0]) // D, m - 2)
        return S.piece(y[j], y[j + 1], Mo[j], Mo[j + 1], (xs - (s + j) * D).astype(dt), D, dt)
    inst, y = short_run_nodes(fm_col, active_col, s, e, D)
    x = inst * D
    if len(x) == 4:
        if dt is np.float64:
            return make_interp_spline(x.astype(np.float64), y, k=3)(xs.astype(np.float64))
        return S.lagrange4(x, y, xs, dt)
    return (lagrange3 if len(x) == 3 else lagrange2)(x, y, xs, dt)


def knot_phases(rec, step, fs, dtype=np.float64):
    """Per slot: code, runs, and for every in-run interval j the local phase sums
    loc[j, u] = sum_{v=1..u} w_j(v) - sum_{v=0..u} sin(pi v/D) er_j (u = 0..D), the unwrapped knot phase R (step 1)
    and the phase of each run's first knot.  `dtype` np.float64 is the definition, np.longdouble the yardstick."""
    return _knot_phases(rec, step, fs, dtype)[:5]


def round_margins(rec, step, fs, dtype=np.longdouble):
    """[n-1, K] float64: |frac(e_j / 2 pi) - 1/2| of every in-run interval (inf elsewhere), the room its whole-turn
    count M_j = rint(e_j / 2 pi) is decided with."""
    return _knot_phases(rec, step, fs, dtype)[5]


def _knot_phases(rec, step, fs, dtype):
    dt = dtype
    n = rec.shape[0]
    K = (rec.shape[1] - 1) // 3
    am, fm, ph = rec[:, :K], rec[:, K:2 * K], rec[:, 2 * K:3 * K].astype(dt)
    D = int(step)
    active = am != 0
    code, runs = run_codes(active)
    two_pi = dt(2.0) * dt(np.pi)
    scale = two_pi / dt(fs)
    ft = np.sin(dt(np.pi) * np.arange(D + 1).astype(dt) / dt(D))
    S_ = np.cumsum(ft)[-1]
    loc = {}
    R = np.zeros((n, K), dt)
    ph0 = np.zeros((n, K), dt)
    margin = np.full((n - 1, K), np.inf)
    for k in range(K):
        tab = np.zeros((n - 1, D + 1), dt)
        for s, e in runs[k]:
            if e == s:
                continue
            dense = _fm_piece_values(fm[:, k], active[:, k], s, e, D, dt)
            nint = e - s
            idx = np.arange(nint)[:, None] * D + np.arange(D + 1)[None, :]
            acc = np.cumsum(scale * dense[idx], axis=1)           # the eval kernel's summation order
            w0 = acc[:, 0]
            shift = ph[s:e, k] - w0
            err = (acc[:, -1] + shift) - ph[s + 1:e + 1, k]
            q = err / two_pi
            Mr = np.rint(q)
            margin[s:e, k] = np.abs((q - np.floor(q)) - dt(0.5)).astype(np.float64)
            er = dt(np.pi) * (err - two_pi * Mr) / dt(2.0 * D)
            er[-1] = (err[-1] - two_pi * Mr[-1]) / S_         # a run's last interval closes its mismatch fully
            c = np.cumsum(ft[None, :] * er[:, None], axis=1)
            tab[s:e] = (acc - w0[:, None]) - c
            delta = (ph[s + 1:e + 1, k] - ph[s:e, k]) + two_pi * Mr
            R[s + 1:e + 1, k] = np.cumsum(delta)
            ph0[s:e + 1, k] = ph[s, k]
        loc[k] = tab
    return code, runs, loc, R, ph0, margin


def locate(Lp, rho, D):
    """(j, r, tau) of the output samples, in float64: the quotient n'/rho is an input of the definition, formed in the
    arithmetic of the kernels, whatever arithmetic the rest of the model runs in."""
    npr = np.arange(Lp, dtype=np.float64)
    tau = npr / rho
    j = np.floor(tau / D).astype(np.int64)
    r = tau - j * float(D)
    lo = r < 0
    j[lo] -= 1
    hi = r >= D
    j[hi] += 1
    r = tau - j * float(D)
    return j, r, tau


def a0_values(a0c, j, tau, n, D, dtype=np.float64):
    """The a0 spline at tau, carried on with its last piece past the last knot."""
    dt = dtype
    if dt is np.float64:
        return make_interp_spline(np.arange(n) * float(D), a0c, k=3)(tau, extrapolate=True)
    y = np.asarray(a0c).astype(dt)
    Mo = S.notaknot_moments(y, D, dt)
    ia = np.clip(j, 0, n - 2)
    return S.piece(y[ia], y[ia + 1], Mo[ia], Mo[ia + 1], tau.astype(dt) - (ia * D).astype(dt), D, dt)


def synthesize(records, step, fs, L, rho=1.0, beta=1.0, preserve_envelope=True, dtype=np.float64):
    dt = dtype
    rec = np.asarray(records, dtype=np.float64)
    n = rec.shape[0]
    K = (rec.shape[1] - 1) // 3
    D = int(step)
    am, fm, ph, a0c = rec[:, :K], rec[:, K:2 * K], rec[:, 2 * K:3 * K], rec[:, 3 * K]
    code, runs, loc, R, ph0 = knot_phases(rec, D, fs, dt)
    Ap = envelope_amplitudes(am, fm, fs, beta, preserve_envelope, dt)
    Lp = int(np.rint(rho * L))
    j, r, tau = locate(Lp, rho, D)
    br = dt(beta) * dt(rho)
    synth = np.zeros(Lp, dt)
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
        cell = np.zeros(Lp, dt)
        if cov.any():
            jj, rr = jk[cov], rk[cov].astype(dt)
            u0 = np.floor(rk[cov]).astype(np.int64)
            fr = rr - u0
            tab = loc[k]
            psi0 = R[jj, k] + tab[jj, u0]
            psi1 = R[jj, k] + tab[jj, np.minimum(u0 + 1, D)]
            phi = ph0[jj, k] + br * ((dt(1.0) - fr) * psi0 + fr * psi1)
            A = ((Ap[jj + 1, k] - Ap[jj, k]) / dt(D)) * rr + Ap[jj, k]
            cell[cov] = np.where(A != 0, A * np.cos(phi), dt(0.0))
        iso = np.flatnonzero(code[:, k] == 1)
        if len(iso):
            ns = np.rint(rho * (iso * float(D))).astype(np.int64)
            keep = (ns >= 0) & (ns < Lp)
            np.add.at(cell, ns[keep], Ap[iso[keep], k] * np.cos(ph[iso[keep], k].astype(dt)))
        synth += cell
    return a0_values(a0c, j, tau, n, D, dt) + dt(2.0) * synth


def records_from_cells(n, K, cells, am, fm, pk, a0):
    """Records from the sparse cell list of a golden fixture (det_cells, det_am, ...)."""
    rec = np.zeros((n, 3 * K + 1))
    i, k = cells[:, 0], cells[:, 1]
    rec[i, k] = am
    rec[i, K + k] = fm
    rec[i, 2 * K + k] = pk
    rec[:, 3 * K] = a0
    return rec
