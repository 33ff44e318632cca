"""NumPy model of the formant tracks: the poles of an all-pole frame by the Aberth-Ehrlich iteration,
the formant candidates among them and the Viterbi decode over the candidates.  Normative for the tests: the kernels of
csrc/eaqhm_formant.hip compute the same thing.  `dt` selects the arithmetic (np.float64: the definition;
np.longdouble: the yardstick the GPU tests take their bars from).  Complex arithmetic is spelled out in real
operations, each rounded once, in the order the kernel takes them."""
from itertools import product

import numpy as np

ITMAX = 64
KC = 8
U = 2.0 ** -53
LD = np.longdouble


def stepup(k, dt=np.float64):
    """[1, a_1, .., a_p] of reflection coefficients k_1..k_p: a_j += k_i a_{i-j}, j = 1..i, from the old values."""
    a = np.zeros(len(k) + 1, dt)
    a[0] = 1
    for i in range(1, len(k) + 1):
        ki = dt(k[i - 1])
        old = a.copy()
        a[1:i + 1] = old[1:i + 1] + ki * old[i - 1::-1][:i]
    return a


def effective_degree(k):
    """pe: the largest i with k_i != 0, 0 if none."""
    nz = np.flatnonzero(np.asarray(k) != 0)
    return int(nz[-1]) + 1 if len(nz) else 0


def horner(a, pe, zr, zi, dt=np.float64):
    """(P, P', s) at z for the monic polynomial a[0..pe], one pass in ascending j; z may be an array (one lane each).
    Returns pr, pi, dr, di, s."""
    zr, zi = np.asarray(zr, dt), np.asarray(zi, dt)
    pr, pi = np.ones_like(zr), np.zeros_like(zr)
    dr, di, s = np.zeros_like(zr), np.zeros_like(zr), np.ones_like(zr)
    az = np.sqrt(zr * zr + zi * zi)
    for j in range(1, pe + 1):
        aj = dt(a[j])
        ndr = (dr * zr - di * zi) + pr
        ndi = (dr * zi + di * zr) + pi
        npr = (pr * zr - pi * zi) + aj
        npi = pr * zi + pi * zr
        dr, di, pr, pi = ndr, ndi, npr, npi
        s = s * az + abs(aj)
    return pr, pi, dr, di, s


def frame_roots(k, dt=np.float64):
    """(roots complex[p] in dt's complex type, iters) of one frame's reflection coefficients."""
    k = np.asarray(k, dtype=np.float64)
    p = len(k)
    pe = effective_degree(k)
    ct = np.complex128 if dt is np.float64 else np.clongdouble
    out = np.zeros(p, ct)
    if pe == 0:
        return out, 0
    a = stepup(k.astype(dt), dt)
    pi_ = dt(np.pi) if dt is np.float64 else 4 * np.arctan(LD(1))
    lane = np.arange(pe).astype(dt)
    r0 = np.exp(np.log(abs(a[pe])) / dt(pe))
    ang = dt(2) * pi_ * lane / dt(pe) + pi_ / (dt(2) * dt(pe))
    zr, zi = r0 * np.cos(ang), r0 * np.sin(ang)
    tol = dt(8.0 * pe * U)
    acc = np.zeros(pe, bool)
    it = 0
    with np.errstate(all="ignore"):
        while True:
            pr, pi, dr, di, s = horner(a, pe, zr, zi, dt)
            acc = acc | (np.sqrt(pr * pr + pi * pi) <= tol * s)
            if acc.all():
                break
            if it == ITMAX:
                it = ITMAX + 1
                break
            den = dr * dr + di * di
            Nr, Ni = (pr * dr + pi * di) / den, (pi * dr - pr * di) / den
            Sr, Si = np.zeros(pe, dt), np.zeros(pe, dt)
            for j in range(pe):
                er, ei = zr - zr[j], zi - zi[j]
                dd = er * er + ei * ei
                qr, qi = er / dd, ei / dd
                other = np.arange(pe) != j
                Sr = np.where(other, Sr + qr, Sr)
                Si = np.where(other, Si - qi, Si)
            wr, wi = dt(1) - (Nr * Sr - Ni * Si), -(Nr * Si + Ni * Sr)
            wd = wr * wr + wi * wi
            cr, ci = (Nr * wr + Ni * wi) / wd, (Ni * wr - Nr * wi) / wd
            zr = np.where(acc, zr, zr - cr)
            zi = np.where(acc, zi, zi - ci)
            it += 1
    out[:pe] = zr + 1j * zi
    return out, it


def roots(refl, dt=np.float64):
    """(roots complex[Nf, p], iters int32[Nf]) of refl float64[Nf, p]."""
    refl = np.asarray(refl, dtype=np.float64)
    got = [frame_roots(row, dt) for row in refl]
    return np.array([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.int32)


def backward_error(k, z):
    """|P(z)| / (pe u s) of every root z[0..pe) of the frame, evaluated in long double (empty for pe = 0)."""
    pe = effective_degree(k)
    if pe == 0:
        return np.zeros(0, LD)
    a = stepup(np.asarray(k, dtype=np.float64).astype(LD), LD)
    z = np.asarray(z)[:pe]
    pr, pi, _, _, s = horner(a, pe, z.real.astype(LD), z.imag.astype(LD), LD)
    return np.sqrt(pr * pr + pi * pi) / (LD(pe) * LD(U) * s)


def candidate_values(roots_, fs, dt=np.float64):
    """(f, b, re, im) in dt for every root of roots complex128[Nf, p]: f = atan2(im, re) fs / (2 pi), b = -ln(sqrt(re^2 +
    im^2)) fs / pi."""
    z = np.asarray(roots_, dtype=np.complex128)
    re, im = z.real.astype(dt), z.imag.astype(dt)
    pi_ = dt(np.pi) if dt is np.float64 else 4 * np.arctan(LD(1))
    with np.errstate(all="ignore"):
        f = np.arctan2(im, re) * dt(fs) / (dt(2) * pi_)
        b = -np.log(np.sqrt(re * re + im * im)) * dt(fs) / pi_
    return f, b, re, im


def candidates(roots_, iters, fs, fmin, fmax, bmax):
    """(f float64[Nf, 8], b float64[Nf, 8], count int32[Nf], index int64[Nf, 8]) of roots complex128[Nf, p]: float64
    arithmetic; index names the root behind every candidate (-1 beyond the count)."""
    f, b, _, im = candidate_values(roots_, fs)
    Nf = f.shape[0]
    f_out, b_out = np.full((Nf, KC), np.nan), np.full((Nf, KC), np.nan)
    count = np.zeros(Nf, np.int32)
    index = np.full((Nf, KC), -1, np.int64)
    for m in range(Nf):
        if iters[m] == ITMAX + 1:
            continue
        ok = np.flatnonzero((im[m] > 0) & (f[m] >= fmin) & (f[m] <= fmax) & (b[m] <= bmax))
        order = ok[np.argsort(f[m][ok], kind="stable")][:KC]          # stable: equal f keeps the lower root index first
        count[m] = len(order)
        f_out[m, :len(order)] = f[m][order]
        b_out[m, :len(order)] = b[m][order]
        index[m, :len(order)] = order
    return f_out, b_out, count, index


def states(N):
    """int8[C(8 + N, N), N]: lexicographic, -1 (absent) first, used indices strictly increasing along the slots."""
    rows = [s for s in product(range(-1, KC), repeat=N)
            if all(x < y for x, y in zip([v for v in s if v >= 0], [v for v in s if v >= 0][1:]))]
    return np.array(rows, dtype=np.int8)


def local_costs(L, count, st, absent):
    """local[t, s]: sum over the slots, in slot order from 0.0; +inf for a state that uses an index >= count[t]."""
    T, N = L.shape[0], L.shape[1]
    idx = st.astype(np.int64)
    out = np.zeros((T, len(st)))
    for n in range(N):
        out = out + np.where(idx[None, :, n] >= 0, L[:, n, :][:, np.maximum(idx[:, n], 0)], absent)
    bad = (idx[None, :, :] >= np.asarray(count)[:, None, None]).any(axis=2)
    return np.where(bad, np.inf, out)


def jump_table(lf, count, t, wj):
    """J float64[9, 9] of the step into t: row and column 0 are "absent"; zero beyond the counts."""
    J = np.zeros((KC + 1, KC + 1))
    ca, cb = min(max(int(count[t - 1]), 0), KC), min(max(int(count[t]), 0), KC)
    J[1:ca + 1, 1:cb + 1] = wj * np.abs(lf[t][None, :cb] - lf[t - 1][:ca, None])
    return J


def forward(L, lf, count, N, wj, absent):
    """dict(q int32[T], bp int16[T, S], last float64[S], total): the decode in float64, first minima throughout."""
    st = states(N)
    idx = st.astype(np.int64) + 1
    T, S = L.shape[0], len(st)
    loc = local_costs(L, count, st, absent)
    D = loc[0].copy()
    bp = np.zeros((T, S), np.int16)
    bp[0] = np.arange(S)
    for t in range(1, T):
        J = jump_table(lf, count, t, wj)
        tr = np.zeros((S, S))
        for n in range(N):
            tr = tr + J[idx[:, n][:, None], idx[:, n][None, :]]
        cand = D[:, None] + tr
        arg = np.argmin(cand, axis=0)                     # the first minimum in state order
        bp[t] = arg
        D = cand[arg, np.arange(S)] + loc[t]
    q = np.zeros(T, np.int32)
    q[T - 1] = int(np.argmin(D))
    for t in range(T - 1, 0, -1):
        q[t - 1] = bp[t, q[t]]
    return dict(q=q, bp=bp, last=D, total=float(D[q[T - 1]]))


def path_cost(L, lf, count, N, wj, absent, q):
    """The total of the state sequence q, summed as the recurrence sums it (inf for an invalid state)."""
    st = states(N)
    idx = st.astype(np.int64) + 1
    loc = local_costs(L, count, st, absent)
    D = loc[0][q[0]]
    for t in range(1, len(q)):
        J = jump_table(lf, count, t, wj)
        tr = 0.0
        for n in range(N):
            tr = tr + J[idx[q[t - 1], n], idx[q[t], n]]
        D = (D + tr) + loc[t][q[t]]
    return D
