"""NumPy model of the interpolation stage (csrc/eaqhm_interp.hip: run codes and spline moments, dense tracks, phase
integration, additive synthesis, error sums) and the generator of the cases the CPU and GPU tests run it on.

Normative for the tests.  It follows oracle/eaqhm_oracle.py::interpolate_tracks and Analysis.post_stage (functions.py:
337-388) operation by operation where the order matters (cumulative sums of the phase, round half to even, numpy.unwrap,
the slots added in slot order) and solves the not-a-knot splines by a plain tridiagonal sweep, so that `dtype` can be
np.float64 (the definition) or np.longdouble (the yardstick the GPU tests take their bars from).

Domain.  Records are (No_ti, 3*Kmax+1): |a_k|, f_k, arg a_k, a0.  A cell is accepted when its amplitude is not zero;
frequency and phase of the other cells are ignored (the kernels do the same: code 0).  Accepted cells lie at instants
[2, No_ti-2]: the reference's run finder (functions.py:352) is not defined outside.  Instant i sits at
sample i*step, and L >= (No_ti-1)*step + 2.
"""
import numpy as np

PI = np.pi                      # the reference's constant: the same double in both arithmetics


# --------------------------------------------------------------------------------------------- splines
def notaknot_moments(y, h, dtype=np.float64):
    """Second derivatives of the not-a-knot cubic through y on knots h apart (len(y) >= 4): M_{i-1} + 4 M_i + M_{i+1} =
    6 (y_{i-1} - 2 y_i + y_{i+1}) / h^2 inside, M_0 = 2 M_1 - M_2 and M_{n-1} = 2 M_{n-2} - M_{n-3} (third derivative
    continuous at the second and the last but one knot), by forward elimination and back substitution."""
    dt = dtype
    y = np.asarray(y).astype(dt)
    n = len(y)
    assert n >= 4
    d = dt(6) * ((y[:-2] - dt(2) * y[1:-1]) + y[2:]) / (dt(h) * dt(h))          # rows 1 .. n-2
    M = np.zeros(n, dt)
    M[1] = d[0] / dt(6)                    # row 1 with M_0 eliminated: 6 M_1 = d_1
    M[n - 2] = d[-1] / dt(6)
    m = n - 4
    if m >= 1:
        # unknowns M_2 .. M_{n-3}: (1, 4, 1) with the known neighbours moved to the right-hand side
        rhs = d[1:-1].copy()
        rhs[0] -= M[1]
        rhs[-1] -= M[n - 2]
        cp = np.zeros(m, dt)
        dp = np.zeros(m, dt)
        cp[0] = dt(1) / dt(4)
        dp[0] = rhs[0] / dt(4)
        for i in range(1, m):
            den = dt(4) - cp[i - 1]
            cp[i] = dt(1) / den
            dp[i] = (rhs[i] - dp[i - 1]) / den
        x = np.zeros(m, dt)
        x[-1] = dp[-1]
        for i in range(m - 2, -1, -1):
            x[i] = dp[i] - cp[i] * x[i + 1]
        M[2:n - 2] = x
    M[0] = dt(2) * M[1] - M[2]
    M[n - 1] = dt(2) * M[n - 2] - M[n - 3]
    return M


def piece(y0, y1, m0, m1, r, h, dt):
    """Cubic piece of a spline interval at offset r from its first knot."""
    u = r / dt(h)
    v = dt(1) - u
    return v * y0 + u * y1 + (dt(h) * dt(h) / dt(6)) * ((v * v * v - v) * m0 + (u * u * u - u) * m1)


def lagrange4(px, py, x, dt):
    """The cubic through four points (the padded case of runs shorter than 4 knots, functions.py:368-371)."""
    px = np.asarray(px).astype(dt)
    py = np.asarray(py).astype(dt)
    x = np.asarray(x).astype(dt)
    out = np.zeros(len(x), dt)
    for p in range(4):
        w = py[p]
        t = np.ones(len(x), dt)
        for q in range(4):
            if q != p:
                w = w / (px[p] - px[q])
                t = t * (x - px[q])
        out = out + w * t
    return out


# --------------------------------------------------------------------------------------------- runs
def runs_of(acc):
    """[(first, last)] of the maximal stretches of consecutive accepted instants (isolated ones included)."""
    idx = np.flatnonzero(acc)
    if len(idx) == 0:
        return []
    cut = np.flatnonzero(np.diff(idx) != 1)
    first = np.concatenate(([idx[0]], idx[cut + 1]))
    last = np.concatenate((idx[cut], [idx[-1]]))
    return list(zip(first.tolist(), last.tolist()))


def unwrap_steps(p, dt):
    """diff(numpy.unwrap(p)) the way numpy computes it, and the distance of every raw step from +-pi."""
    dd = np.diff(p)
    two_pi = dt(2) * dt(PI)
    ddmod = np.mod(dd + dt(PI), two_pi) - dt(PI)
    ddmod[(ddmod == -dt(PI)) & (dd > 0)] = dt(PI)
    corr = ddmod - dd
    corr[np.abs(dd) < dt(PI)] = 0
    up = p.copy()
    up[1:] = p[1:] + np.cumsum(corr)
    return np.diff(up), np.abs(np.abs(dd) - dt(PI)).astype(np.float64)


def phase_integrate(omega, ph, knots, dtype=np.float64, margins=None):
    """phase_integr_interpolation (functions.py:537-575) for knots of any spacing: the dense phase on
    [knots[0], knots[-1]].  `margins`, a list, receives the distance of e / 2 pi from a half-integer per interval."""
    dt = dtype
    omega = np.asarray(omega).astype(dt)
    ph = np.asarray(ph).astype(dt)
    two_pi = dt(2) * dt(PI)
    out = np.zeros(len(omega), dt)
    for i in range(len(knots) - 1):
        i0, i1 = int(knots[i]), int(knots[i + 1])
        p = np.cumsum(omega[i0:i1 + 1])
        p = p + (ph[i0] - p[0])
        e = p[-1] - ph[i1]
        q = e / two_pi
        M = np.round(q)
        if margins is not None:
            margins.append(float(abs((q - np.floor(q)) - dt(0.5))))
        er = dt(PI) * (e - two_pi * M) / dt(2 * (i1 - i0))
        tt = np.arange(0, i1 - i0 + 1).astype(dt)
        p = p - np.cumsum(np.sin(dt(PI) * tt / dt(i1 - i0)) * er)
        out[i0:i1 + 1] = p
    return out[int(knots[0]):int(knots[-1]) + 1]


# --------------------------------------------------------------------------------------------- the stage
def interpolate(records, step, fs, L, target=None, std_det=None, dtype=np.float64):
    """The whole stage from frame-centre records.  Returns a dict:
      am, fm_next, fm_recon, ph   (L, Kmax) dense amplitude, next-iteration frequency (functions.py:375), interpolated
                                  frequency and phase; zero outside runs (an isolated instant keeps am and ph, fm_next 0)
      ph_knot (No_ti, Kmax), a0 (L,), s_hat (L,) = a0 + 2 sum_k am cos(ph), slots added in slot order
      sum_d, sum_d2, srer         over the whole signal against `target` (population std; std_det = std(target))
      code (No_ti, Kmax) uint8, mom (No_ti, Kmax+1)   the kernels' tables: 0 / 1 / 2 / 16 + 4 m + pos; second
                                  derivatives on the knots of runs of >= 4 (zero elsewhere), the a0 spline last
      margin_round (No_ti, Kmax)  per interval starting at the instant: |frac(e / 2 pi) - 1/2| (inf where none)
      margin_unwrap (L, Kmax)     per sample: | |phase step into the sample| - pi | (inf where none)"""
    dt = dtype
    rec = np.asarray(records, dtype=np.float64)
    No_ti = rec.shape[0]
    K = (rec.shape[1] - 1) // 3
    D = int(step)
    assert No_ti >= 4 and (No_ti - 1) * D + 2 <= L
    acc = rec[:, :K] != 0
    assert not acc[:2].any() and not acc[No_ti - 1:].any(), "accepted cells outside instants [2, No_ti-2]"
    am_c = rec[:, :K].astype(dt)
    fm_c = np.where(acc, rec[:, K:2 * K], 0.0).astype(dt)
    ph_c = np.where(acc, rec[:, 2 * K:3 * K], 0.0).astype(dt)
    a0_c = rec[:, 3 * K].astype(dt)
    two_pi = dt(2) * dt(PI)
    scale = two_pi / dt(fs)
    unscale = dt(fs) / two_pi
    am = np.zeros((L, K), dt)
    fm_recon = np.zeros((L, K), dt)
    ph = np.zeros((L, K), dt)
    fm_next = np.zeros((L, K), dt)
    code = np.zeros((No_ti, K), np.uint8)
    mom = np.zeros((No_ti, K + 1), dt)
    margin_round = np.full((No_ti, K), np.inf)
    margin_unwrap = np.full((L, K), np.inf)
    r = np.arange(D + 1).astype(dt)
    ft = np.sin(dt(PI) * r / dt(D))
    for k in range(K):
        for i0, i1 in runs_of(acc[:, k]):
            m = i1 - i0 + 1
            if m == 1:
                code[i0, k] = 1
                am[i0 * D, k] = am_c[i0, k]
                ph[i0 * D, k] = ph_c[i0, k]
                fm_recon[i0 * D, k] = fm_c[i0, k]
                continue
            t_a, t_b = i0 * D, i1 * D
            x = np.arange(t_a, t_b + 1)
            # amplitude: linear between the knots (functions.py:364; numpy.interp's formula)
            j = np.minimum((x - t_a) // D, m - 2)
            ya, yb = am_c[i0 + j, k], am_c[i0 + j + 1, k]
            xa = ((i0 + j) * D).astype(dt)
            a_lin = ((yb - ya) / dt(D)) * (x.astype(dt) - xa) + ya
            a_lin[-1] = am_c[i1, k]
            am[t_a:t_b + 1, k] = a_lin
            # frequency: cubic (functions.py:367-371)
            if m >= 4:
                code[i0:i1 + 1, k] = 2
                M = notaknot_moments(fm_c[i0:i1 + 1, k], D, dt)
                mom[i0:i1 + 1, k] = M
                y = fm_c[i0:i1 + 1, k]
                rr = (x - (i0 + j) * D).astype(dt)
                f = piece(y[j], y[j + 1], M[j], M[j + 1], rr, D, dt)
            else:
                code[i0:i1 + 1, k] = 16 + 4 * m + np.arange(m)
                npad = 4 - m
                pad = np.arange(npad)
                px = np.concatenate((pad * D, np.arange(i0, i1 + 1) * D))
                py = np.concatenate((fm_c[pad, k], fm_c[i0:i1 + 1, k]))      # whatever the pad instants hold
                f = lagrange4(px, py, x, dt)
            fm_recon[t_a:t_b + 1, k] = f
            # phase: integrate the frequency per interval, close the error with a sine bump (functions.py:537-575)
            om = scale * f
            idx = (np.arange(m - 1) * D)[:, None] + np.arange(D + 1)[None, :]
            p = np.cumsum(om[idx], axis=1)
            p = p + (ph_c[i0:i1, k] - p[:, 0])[:, None]
            e = p[:, -1] - ph_c[i0 + 1:i1 + 1, k]
            q = e / two_pi
            Mr = np.round(q)                                                  # half to even
            margin_round[i0:i1, k] = np.abs((q - np.floor(q)) - dt(0.5)).astype(np.float64)
            er = dt(PI) * (e - two_pi * Mr) / dt(2 * D)
            p = p - np.cumsum(ft[None, :] * er[:, None], axis=1)
            dense = np.empty(t_b - t_a + 1, dt)
            dense[idx[:, :-1].ravel()] = p[:, :-1].ravel()
            dense[-1] = p[-1, -1]                                             # the last knot keeps the integrated value
            ph[t_a:t_b + 1, k] = dense
            steps, mg = unwrap_steps(dense, dt)
            fm_next[t_a, k] = f[0]
            fm_next[t_a + 1:t_b + 1, k] = unscale * steps
            margin_unwrap[t_a + 1:t_b + 1, k] = mg
    # a0: not-a-knot spline through every instant, the last piece carried on past the last instant (functions.py:340)
    Ma = notaknot_moments(a0_c, D, dt)
    mom[:, K] = Ma
    t = np.arange(L)
    ia = np.minimum(t // D, No_ti - 2)
    a0 = piece(a0_c[ia], a0_c[ia + 1], Ma[ia], Ma[ia + 1], (t - ia * D).astype(dt), D, dt)
    synth = np.zeros(L, dt)
    for k in range(K):                                                        # slot order
        synth = synth + np.where(am[:, k] != 0, am[:, k] * np.cos(ph[:, k]), dt(0))
    s_hat = a0 + dt(2) * synth
    c = np.arange(No_ti) * D
    out = dict(am=am, fm_next=fm_next, fm_recon=fm_recon, ph=ph, ph_knot=ph[c].copy(), a0=a0, s_hat=s_hat, code=code,
               mom=mom, margin_round=margin_round, margin_unwrap=margin_unwrap)
    if target is not None:
        tg = np.asarray(target, dtype=np.float64)
        d = tg.astype(dt) - s_hat
        mean = d.sum() / dt(L)
        sd = np.sqrt(((d - mean) * (d - mean)).sum() / dt(L))
        sdet = dt(np.std(tg) if std_det is None else std_det)
        with np.errstate(all="ignore"):
            out.update(sum_d=d.sum(), sum_d2=(d * d).sum(), srer=dt(20) * np.log10(sdet / sd))
    return out


def excluded_cells(ref, step, margin=1e-9):
    """(L, Kmax) bool: cells whose value hangs on a decision the reference itself takes with less than `margin` to
    spare: the samples of an interval whose e / 2 pi is that close to a half-integer, and a sample whose phase step is
    that close to +-pi."""
    L, K = ref["am"].shape
    bad = ref["margin_unwrap"] < margin
    for i, k in zip(*np.nonzero(ref["margin_round"] < margin)):
        bad[i * step:(i + 1) * step + 1, k] = True
    return bad


# --------------------------------------------------------------------------------------------- error sums
ES_SHIFT_MAX = 900


def error_sum_shift(std_det):
    """The power of two the error is scaled by before it is summed (include/eaqhm_hip.h): 10 - e of std_det = m 2^e,
    0.5 <= m < 1; 0 for a std_det that is zero or not finite."""
    s = float(std_det)
    if not (s > 0.0) or not np.isfinite(s):
        return 0
    return int(np.clip(10 - np.frexp(s)[1], -ES_SHIFT_MAX, ES_SHIFT_MAX))


def fixed_point_sums(d, std_det, rounding=np.rint):
    """The header's fixed-point contract on float64 errors d, in Python integers: (sum rint(d' 2^60),
    sum rint(d'^2 2^64), count of samples with |d'| >= 2^30 or not finite, shift), d' = d 2^shift."""
    sh = error_sum_shift(std_det)
    dp = np.ldexp(np.asarray(d, dtype=np.float64), sh)
    with np.errstate(invalid="ignore"):
        ok = np.abs(dp) < 2.0 ** 30
    g = dp[ok]
    tot = sum(int(v) for v in rounding(np.ldexp(g, 60)))
    tot2 = sum(int(v) for v in rounding(np.ldexp(g * g, 64)))
    return tot, tot2, int(np.count_nonzero(~ok)), sh


def limbs_of(tot, tot2, bad, shift):
    """One cut of the two integers into the eight words of sums_out[8..15] (any cut that adds up to them serves)."""
    out = []
    for v in (tot, tot2):
        out += [v & 0xffffffff, (v >> 32) & 0xffffffff, v >> 64]
    return out + [bad, shift]


def ints_of(limbs):
    """(sum d' 2^60, sum d'^2 2^64, count, shift) from eight int64 words."""
    v = [int(x) for x in limbs]
    return v[0] + (v[1] << 32) + (v[2] << 64), v[3] + (v[4] << 32) + (v[5] << 64), v[6], v[7]


# --------------------------------------------------------------------------------------------- launch geometry
def eval_block_samples(Kmax, step):
    """Samples per block of eaqhm_eval_kernel and its LDS bytes: the largest of 64 / 32 / 16 whose tables fit 78 KiB
    (csrc/eaqhm_interp.hip, eval_block_samples)."""
    for tbs in (64, 32, 16):
        NK, NR = tbs // step + 2, tbs // step + 5
        b = ((step + 2) & ~1) * 8 + (2 * Kmax * (tbs + 1) + Kmax * NK) * 8 + NR * ((3 * Kmax + 1) + (Kmax + 1)) * 8 + \
            ((NR * Kmax + 7) & ~7)
        if b <= 78 * 1024 or tbs == 16:
            return tbs, b
    raise AssertionError


# --------------------------------------------------------------------------------------------- cases
RUN_LENGTHS = [1, 2, 3, 4, 5, 6] + list(range(38, 43)) + list(range(75, 86)) + [200, 230]


def _pack(No_ti, K, lengths, rng):
    """Accepted mask (No_ti, K) inside instants [2, No_ti-2].  Slot 0: nothing; slot 1: every instant of the domain;
    slot 2: short runs behind accepted instants 2..3 (a run 2..3, then runs of 2 and 3 knots); slot 3: the same short
    runs with instants 2..3 empty, a run ending at No_ti-2; slot 4: a run starting at instant 2 and two runs one
    rejected instant apart; the other slots: `lengths` dealt out in turn, 1 to 3 rejected instants between runs."""
    acc = np.zeros((No_ti, K), bool)
    lo, hi = 2, No_ti - 2
    acc[lo:hi + 1, 1] = True
    if K > 2:
        for s, n in ((2, 2), (6, 2), (10, 3), (15, 1), (17, 3), (21, 2)):
            if s + n - 1 <= hi:
                acc[s:s + n, 2] = True
    if K > 3:
        for s, n in ((6, 2), (10, 3), (15, 1), (17, 3), (21, 2)):
            if s + n - 1 <= hi:
                acc[s:s + n, 3] = True
        n = min(5, hi - 24)
        if n >= 2:
            acc[hi - n + 1:hi + 1, 3] = True
    if K > 4:
        n = min(7, hi - lo + 1)
        acc[lo:lo + n, 4] = True
        if lo + n + 1 + 4 <= hi:
            acc[lo + n + 1:lo + n + 5, 4] = True                     # one rejected instant apart
    pos = [lo + int(rng.integers(0, 3)) for _ in range(K)]
    k = 5
    for n in sorted(lengths, reverse=True):
        if K <= 5:
            break
        tries = 0
        while pos[k] + n - 1 > hi and tries < K:
            k = 5 + (k - 4) % (K - 5)
            tries += 1
        if pos[k] + n - 1 > hi:
            continue                                                 # does not fit this geometry
        acc[pos[k]:pos[k] + n, k] = True
        pos[k] += n + int(rng.integers(1, 4))
        k = 5 + (k - 4) % (K - 5)
    return acc


def _values(acc, fs, rng, dirty=False):
    """Records for an accepted mask: amplitudes over 6 decades, phases uniform in (-pi, pi], frequencies smooth along
    time (slot 1 up to 200 Hz under Nyquist, the last slot white), a0 smooth plus noise.  dirty: the frequency and
    phase of the cells that are not accepted hold leftovers instead of zeros."""
    No_ti, K = acc.shape
    x = np.arange(No_ti) / max(No_ti - 1, 1)
    rec = np.zeros((No_ti, 3 * K + 1))
    nyq = fs / 2.0
    for k in range(K):
        # slot 1 at level 1 and slot 2 at 10^-6.3, the others anywhere between: 6 decades between accepted cells
        level = 10.0 ** rng.uniform(-6, 0) if k > 2 else (0.5, 1.0, 10.0 ** -6.3)[k]
        amp = level * (1.0 + 0.5 * np.sin(2 * np.pi * (rng.uniform(0.5, 3) * x + rng.uniform())))
        base = rng.uniform(80.0, 0.8 * nyq)
        fm = base * (1.0 + 0.03 * np.sin(2 * np.pi * (rng.uniform(0.5, 4) * x + rng.uniform()))) \
            + 2.0 * rng.standard_normal(No_ti)
        if k == 1:
            fm = nyq - 200.0 - 150.0 * (1.0 + np.sin(2 * np.pi * (1.5 * x + 0.1)))
        if k == K - 1 and K > 5:
            fm = 0.4 * nyq + 0.05 * nyq * rng.standard_normal(No_ti)
        ph = -rng.uniform(-np.pi, np.pi, No_ti)                       # (-pi, pi]
        a = acc[:, k]
        rec[a, k] = amp[a]
        if dirty:
            rec[:, K + k] = fm
            rec[:, 2 * K + k] = ph
        else:
            rec[a, K + k] = fm[a]
            rec[a, 2 * K + k] = ph[a]
    rec[:, 3 * K] = 0.01 * np.sin(2 * np.pi * 2.3 * x) + 0.003 * rng.standard_normal(No_ti)
    return rec


def make_case(name, No_ti, K, step, fs, extra=0, lengths=RUN_LENGTHS, seed=0, dirty=False):
    """One named case: dict(name, records, No_ti, Kmax, step, fs, L, target).  L = (No_ti-1)*step + 2 + extra."""
    rng = np.random.default_rng([seed, No_ti, K, step, int(fs)])
    acc = _pack(No_ti, K, lengths, rng)
    rec = _values(acc, fs, rng, dirty)
    L = (No_ti - 1) * step + 2 + extra
    target = 0.3 * rng.standard_normal(L)
    return dict(name=name, records=rec, No_ti=No_ti, Kmax=K, step=step, fs=fs, L=L, target=target, dirty=dirty)


SHORT = [1, 2, 3, 4, 5, 6] + list(range(38, 43))


def cases():
    """The named cases (same seed, same cases).  Block size of eaqhm_eval_kernel in the name: b64 / b32 / b16."""
    return [
        make_case("b32_s15_k59_16k", 300, 59, 15, 16000),
        make_case("b64_s7_k12_48k_past", 300, 12, 7, 48000, extra=7),
        make_case("b64_s1_k12_16k", 300, 12, 1, 16000),
        make_case("b16_s15_k120_16k_past", 300, 120, 15, 16000, extra=15),
        make_case("b32_s80_k70_48k", 300, 70, 80, 48000, extra=3),
        make_case("b64_s240_k12_48k_past", 300, 12, 240, 48000, extra=240),
        make_case("b16_s240_k120_16k", 60, 120, 240, 16000, lengths=SHORT),
        make_case("b64_n4", 4, 3, 15, 16000, lengths=[]),
        make_case("b64_n5", 5, 3, 15, 16000, lengths=[]),
        make_case("b64_n6_past", 6, 3, 15, 16000, extra=15, lengths=[]),
        make_case("b64_s15_k12_dirty", 120, 12, 15, 16000, lengths=SHORT, dirty=True),
    ]


def clean_records(case):
    """The records with the cells that are not accepted zeroed (what the reference's arrays hold)."""
    rec = case["records"].copy()
    K = case["Kmax"]
    off = rec[:, :K] == 0
    rec[:, K:2 * K][off] = 0
    rec[:, 2 * K:3 * K][off] = 0
    return rec


def run_lengths(acc):
    """Sorted list of the run lengths of a mask (every slot)."""
    out = []
    for k in range(acc.shape[1]):
        out += [b - a + 1 for a, b in runs_of(acc[:, k])]
    return sorted(out)
