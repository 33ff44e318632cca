"""Case tables and input builders of the direct tests of the cepstrum kernels (csrc/eaqhm_cepstrum.hip; DESIGN.md §9.5,
§9.7, §9.8): the fit, the amplitude readout, the envelope and phase grid readouts and the model build, each on the linear
axis and on the all-pass warped one, at every node count, order and grid edge of the kernels.  Plain NumPy, no torch:
tests/test_cepstrum_direct_cases_cpu.py shows with the models alone that the cases can judge a kernel,
tests/test_gpu_cepstrum_direct.py runs them on the device through the context's raw entry points.

The models are tests/model_cepstrum_ref.py, tests/cepstrum_warp_ref.py and tests/model_build_ref.py.  `*_models(...)` runs
the model of one call in float64 (the definition) and in np.longdouble; the deviation between the two is the yardstick
from which the GPU test takes its bar (100 x, DESIGN.md §10's rule).  A case is one call.  For the fit that is one launch
per (K, P, lam, axis), which carries every activity pattern as its instants: its yardstick is the largest deviation of
any of them, and `dev` keeps the deviation of each for the record.  (An instant alone is no case: the two coefficients
of an instant at order 1 deviate by 9.6e-12 on the `first` pattern and by 1.3e-13 on `last` at K = 128, two single-node
instants of one structure, and by less than half an ulp where float64 happens to round to the long double value.)  The
models of a call are computed once per process.

An axis is None (the plain entry point) or the coefficient a of the `_warped` entry point."""
import numpy as np

import cepstrum_warp_ref as CW
import model_build_ref as MB
import model_cepstrum_ref as CR

FS = 16000.0
AXES = [None, 0.42, -0.9]
CEP_WAVES = 4                     # instants or rows per block, one wave each
CEP_PMAX = 63
CEPSTRUM_LDS_MAX = 160 * 1024     # bytes of dynamic LDS the fit's launch accepts
DENORMAL = 5e-324


def axis_name(a):
    return "lin" if a is None else "a%g" % a


def _pair(ref, ref_l):
    return float(np.abs(ref - ref_l).max()) if np.size(ref) else 0.0


def wrapped(d):
    """A phase difference mod 2 pi, in [-pi, pi): a value next to +-pi may land on either side."""
    d = np.asarray(d)
    pi = CR._pi(d.dtype.type)
    return d - 2 * pi * np.floor((d + pi) / (2 * pi))


_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- the fit's LDS: csrc/eaqhm_cepstrum.hip's cep_stride and cep_wave_doubles
def cep_stride(P):
    return (P + 1) | 1


def cep_wave_doubles(K, P):
    return 2 * K + (2 * P + 2) + (P + 1) * cep_stride(P)


def fit_lds_bytes(K, P):
    return CEP_WAVES * cep_wave_doubles(K, P) * 8


LDS_ACCEPTED = [(416, 63), (2555, 1)]     # the largest Kmax the launch accepts at the largest and the smallest order
LDS_REFUSED = [(417, 63), (2556, 1)]


# ---- 1. the fit
FIT_K = [1, 2, 63, 64, 65, 128, 129, 416]
FIT_P = [1, 2, 31, 32, 33, 62, 63]
FIT_LAMS = [1e-6, 5e-4, 1.0]
FIT_COUNTS = [1, 4, 5]
FIT_PATTERNS = ["full", "holes", "first", "last", "chunk1_off", "tied", "above_nyquist", "denormal", "empty",
                "full_again"]


def fit_patterns(K):
    """The instants of a launch, in order, where K allows them: ten for K >= 65, nine for 2 <= K <= 64 (no slots 64..127),
    five for K = 1; never a multiple of the four waves of a block, so the last block is part-filled."""
    if K == 1:
        return ["full", "above_nyquist", "denormal", "empty", "full_again"]
    return [p for p in FIT_PATTERNS if K >= 65 or p != "chunk1_off"]


def ln_am(f, shift=0.0):
    """A smooth formant-like log amplitude over frequency (Hz)."""
    return (-3.0 - f / 5000.0 + 2.0 * np.exp(-((f - 700.0 - shift) / 300.0) ** 2)
            + 1.5 * np.exp(-((f - 2400.0) / 500.0) ** 2))


def node_frequencies(K, fs=FS, seed=11):
    """K sorted random frequencies in (40 Hz, fs/2 - 100 Hz), no two equal."""
    f = np.sort(np.random.default_rng([seed, K]).uniform(40.0, fs / 2 - 100.0, K))
    assert len(np.unique(f)) == K
    return f


def pattern_row(K, pattern, fs=FS, seed=11):
    """(am [K], fm [K]) of one instant.  holes: about 40 % of the slots inactive, alternately by am == 0 and by f <= 0
    (0 and -f in turn) with am != 0, slot 0 and slot K - 1 kept active; first, last: one active slot, the others off by
    am == 0; chunk1_off: slots 64..127 off; tied: two equal frequencies (three from K = 4); above_nyquist: the last node
    at 0.55 fs; denormal: am of slot K // 3 at 5e-324; empty: every slot off, even ones by am, odd ones by f."""
    f = node_frequencies(K, fs, seed)
    am = np.exp(ln_am(f) + 0.1 * np.sin(1.3 * np.arange(K)))
    rng = np.random.default_rng([seed, K, FIT_PATTERNS.index(pattern)])
    if pattern == "holes":
        off = np.flatnonzero(rng.random(K) < 0.4)
        off = off[(off != 0) & (off != K - 1)]
        am[off[0::2]] = 0.0
        f[off[1::4]] = 0.0
        f[off[3::4]] = -f[off[3::4]]
    elif pattern == "first":
        am[1:] = 0.0
    elif pattern == "last":
        am[:-1] = 0.0
    elif pattern == "chunk1_off":
        am[64:128:2] = 0.0
        f[65:128:2] = 0.0
    elif pattern == "tied":
        f[K // 2] = f[K // 2 - 1]
        if K >= 4:
            f[K // 2 + 1] = f[K // 2 - 1]
    elif pattern == "above_nyquist":
        f[K - 1] = 0.55 * fs
    elif pattern == "denormal":
        am[K // 3] = DENORMAL
    elif pattern == "empty":
        am[0::2] = 0.0
        f[1::2] = 0.0
    elif pattern == "full_again":
        am = am * 1.0
    else:
        assert pattern == "full", pattern
    return am, f


def records_of(rows):
    """The records [n][3 K + 1] of (am, fm) rows: phases and a0 are not read by the kernels under test."""
    K = len(rows[0][0])
    rec = np.zeros((len(rows), 3 * K + 1))
    for i, (am, f) in enumerate(rows):
        rec[i, :K], rec[i, K:2 * K] = am, f
        rec[i, 2 * K:3 * K] = 0.1 * np.arange(K)
        rec[i, 3 * K] = 0.001 * i
    return rec


def fit_records(K, fs=FS):
    return _once(("fit_records", K, fs), lambda: records_of([pattern_row(K, p, fs) for p in fit_patterns(K)]))


def active_slots(rec):
    K = (rec.shape[1] - 1) // 3
    return (rec[:, :K] != 0) & (rec[:, K:2 * K] > 0)


def model_fit(rec, fs, P, lam, a, dtype=np.float64):
    return CR.fit(rec, fs, P, lam, dtype) if a is None else CW.fit(rec, fs, P, lam, a, dtype)


def fit_models_of(key, rec, fs, P, lam, a):
    """dict(c, c_l, empty [n], dev [n], dev_case): per instant the largest coefficient deviation (0 on an empty instant,
    whose row is exact), and the largest of them, the launch's yardstick."""
    def make():
        c, c_l = model_fit(rec, fs, P, lam, a), model_fit(rec, fs, P, lam, a, np.longdouble)
        empty = ~active_slots(rec).any(axis=1)
        dev = np.zeros(len(rec))
        dev[~empty] = np.abs(c[~empty] - c_l[~empty]).max(axis=1).astype(np.float64)
        return dict(c=c, c_l=c_l, empty=empty, dev=dev, dev_case=float(dev.max()))
    return _once(("fit",) + tuple(key) + (fs, P, lam, a), make)


def fit_models(K, P, lam, a):
    return fit_models_of(("table", K), fit_records(K), FS, P, lam, a)


def lds_records(K):
    """Two instants at an LDS-ceiling K: every slot active, and about 40 % holes."""
    return _once(("lds_records", K), lambda: records_of([pattern_row(K, "full"), pattern_row(K, "holes")]))


# ---- 3. the breakdown of the factorisation
# (order, axis): without the penalty's help the good instants must factor on their own, which at a = -0.9 (the nodes
# crowd into the top of the warped axis: condition 2e8 at order 3, 2e11 at order 4) they do up to order 3
BREAK_CASES = [(P, a) for a in AXES for P in ((1, 2, 8) if a != -0.9 else (1, 2, 3))]
BREAK_K = 40
BREAK_LAM = 1e-300
BREAK_F = 1e-300


def breakdown_records():
    """Eight good instants (two blocks) and the bad row.  The good ones have 20 nodes or more each, so that they factor
    at lam = 1e-300 without the penalty's help (BREAK_CASES).  The bad row has one node, at 1e-300 Hz: every cos(d w)
    is exactly 1, so G_00 = 1, G_10 = 2, G_11 = 4 + 8 pi^2 1e-300 = 4 and pivot 1 = 4 - 2 * 2 is exactly 0."""
    pats = ("full", "holes", "tied", "denormal", "above_nyquist", "full", "holes", "tied")
    good = records_of([pattern_row(BREAK_K, p, seed=23 + i) for i, p in enumerate(pats)])
    assert active_slots(good).sum(axis=1).min() >= 20
    am, f = np.zeros(BREAK_K), np.zeros(BREAK_K)
    am[2], f[2] = 0.37, BREAK_F
    return good, records_of([(am, f)])[0]


def first_pivots(rec_row, fs, lam, a):
    """(G_00, G_10, G_11, pivot 1) of one instant in float64, by the kernel's formulas from T_d = sum cos(d w_n)."""
    K = (len(rec_row) - 1) // 3
    w, _ = CR.nodes(rec_row[:K], rec_row[K:2 * K], fs) if a is None else CW.nodes(rec_row[:K], rec_row[K:2 * K], fs, a)
    T = [float(np.cos(d * w).sum()) for d in range(3)]
    g00, g10 = T[0], 2.0 * T[1]
    g11 = 2.0 * (T[0] + T[2]) + lam * (8.0 * np.pi * np.pi)
    l10 = g10 / np.sqrt(g00)
    return g00, g10, g11, g11 - l10 * l10


# ---- 4. the grid readouts
GRID_N = [1, 3, 4, 5, 9]
GRID_F = [1, 63, 64, 65, 129]
GRID_P = [1, 2, 32, 63]
GRID_B = [1, 2, 16]
GRID_ALPHAS = [0.25, 1.0, 4.0]
GRID_MODES = ["none", "alpha0.25", "alpha1", "alpha4", "alpha_rows", "map_B1", "map_B2", "map_B16"]
EMPTY_ROWS = {1: (), 3: (2,), 4: (3,), 5: (2, 4), 9: (1, 4, 6, 7)}     # n = 9: wave positions 1, 0, 2, 3


def grid_shapes():
    """(n, F, P): every n at F = 65 and every F at n = 9 at the smallest and the largest order, the other orders at
    (9, 129) and (5, 64)."""
    pairs = [(n, 65) for n in GRID_N] + [(9, F) for F in GRID_F if F != 65]
    return [(n, F, P) for P in (1, 63) for n, F in pairs] + [(n, F, P) for P in (2, 32) for n, F in ((9, 129), (5, 64))]


def grid_rows(n, P, a):
    """The model's own float64 fits (lam = 5e-4, on the axis a) of n instants of 40 harmonics of 190 Hz whose first
    formant moves with the instant; the rows of EMPTY_ROWS[n] are the empty row (-inf, 0, .., 0)."""
    def make():
        f = 190.0 * np.arange(1, 41)
        rows = [(np.exp(ln_am(f, 40.0 * i)), f) if i not in EMPTY_ROWS[n] else (np.zeros(40), f) for i in range(n)]
        C = model_fit(records_of(rows), FS, P, 5e-4, a)
        assert np.array_equal(np.isneginf(C[:, 0]), np.isin(np.arange(n), EMPTY_ROWS[n]))
        return C
    return _once(("grid_rows", n, P, a), make)


def grid_map(n, B):
    """(x [B], y [n, B]) in Hz, row n // 3 the identity (x bit for bit), no other row.  B = 1: one breakpoint at
    0.3 fs moved by -20 .. +16 %; B = 2, 16: noise_direct_cases.warp_map's, the last breakpoint (fs/2, fs/2)."""
    nyq = FS / 2
    u = np.linspace(-1.0, 0.8, n)[:, None] if n > 1 else np.array([[1.0]])
    if B == 1:
        x = np.array([0.3 * FS])
        y = (1.0 + 0.2 * u) * x[0]
    elif B == 2:
        x = np.array([0.7 * nyq, nyq])
        y = np.concatenate(((1.0 + 0.2 * u) * x[0], np.full((n, 1), nyq)), axis=1)
    else:
        j = np.arange(1, B + 1)
        x = nyq * j / B
        y = x * (1.0 + 0.15 * u * np.sin(np.pi * j / B))
        y[:, -1] = nyq
    y = np.ascontiguousarray(np.broadcast_to(y, (n, B)), dtype=np.float64).copy()
    if n > 1:
        y[n // 3] = x
    assert np.all(np.diff(np.concatenate((np.zeros((n, 1)), y), axis=1), axis=1) > 0)
    return x, y


def knot_row(n):
    """The row whose knots the grid carries: the last one that is neither the identity nor (n = 9) an empty row."""
    return max(i for i in range(n) if i not in EMPTY_ROWS[n] and (n == 1 or i != n // 3))


def grid_freqs(F, n):
    """F frequencies in Hz.  F = 1: fs/2 alone.  Otherwise 0, fs/2 exactly, its float64 neighbours on both sides,
    0.6 fs, every knot y_j of row knot_row(n) of the three maps (where V changes its segment) with both float64
    neighbours, then seeded random points in [0, 0.55 fs] up to F; in a seeded random order."""
    if F == 1:
        return np.array([FS / 2])
    nyq = FS / 2
    pts = [0.0, nyq, np.nextafter(nyq, 0.0), np.nextafter(nyq, np.inf), 0.6 * FS]
    knots = []
    for B in GRID_B:
        knots += list(grid_map(n, B)[1][knot_row(n)])
    for k in knots:
        for v in (k, np.nextafter(k, 0.0), np.nextafter(k, np.inf)):
            if v not in pts:
                pts.append(v)
    assert len(pts) <= 63, len(pts)
    rng = np.random.default_rng([F, n])
    pts = np.concatenate((pts, rng.uniform(0.0, 0.55 * FS, F - len(pts))))
    return rng.permutation(pts)


def grid_mode(mode, n):
    """(alpha [n] or None, (x, y) or None) of a read mode; the contour runs 0.3 .. 3.5 with exact 1.0 at rows 0, 3, 6
    (0.6 for a single row)."""
    if mode == "none":
        return None, None
    if mode == "alpha_rows":
        al = np.geomspace(0.3, 3.5, n)
        al[0::3] = 1.0
        if n == 1:
            al[0] = 0.6
        return al, None
    if mode.startswith("alpha"):
        return np.full(n, float(mode[5:])), None
    return None, grid_map(n, int(mode[5:]))


def model_series(C, fs, q, a, dtype=np.float64):
    """(C, Phi) [n, F] at the read frequencies q [n, F] (held inside): the direct sums of cepstrum_warp_ref.series on
    the warped axis; on the linear one the envelope of model_cepstrum_ref.readout and the phase of
    model_build_ref.series."""
    fin = np.where(np.isfinite(C), C, 0.0)
    if a is None:
        return CR.readout(C, fs, q, dtype), MB.series(fin, fs, q, dtype)[1]
    return CW.readout(C, fs, q, a, dtype), CW.series(fin, fs, q, a, dtype)[1]


def grid_models(n, F, P, a, mode):
    """dict(env, env_l, ph, ph_l, dev_env, dev_ph, empty [n]): the deviations over the non-empty rows, the phase's as a
    wrapped difference."""
    def make():
        C = grid_rows(n, P, a)
        alpha, warp = grid_mode(mode, n)
        q = CR.read_frequency(grid_freqs(F, n), n, alpha, warp)
        with np.errstate(invalid="ignore"):
            (env, ph), (env_l, ph_l) = model_series(C, FS, q, a), model_series(C, FS, q, a, np.longdouble)
        empty = np.isneginf(C[:, 0])
        return dict(env=env, env_l=env_l, ph=ph, ph_l=ph_l, empty=empty, dev_env=_pair(env[~empty], env_l[~empty]),
                    dev_ph=float(np.abs(wrapped(ph[~empty] - ph_l[~empty])).max()))
    return _once(("grid", n, F, P, a, mode), make)


# ---- 5. the amplitude readout
AMP_COUNTS = [4, 5, 9]
AMP_K = [1, 63, 64, 65, 129]
AMP_P = [1, 63]
AMP_MODES = ["none", "alpha_rows", "map_B16"]
AMP_BETA = 1.25
AMP_F_EDGE = 6400.0        # 1.25 * 6400 == 8000 == fs/2 exactly; 1.25 * nextafter(6400, 0) == nextafter(8000, 0)


def amp_case(n, K):
    """dict(rec, beta [n], edge [n], below [n]): instant i takes the pattern i of fit_patterns(K) (in turn), then one of
    its active slots (edge[i], the last one) gets f = 6400 Hz on even instants, so that beta f == fs/2 exactly, and the
    lower float64 neighbour of 6400 on odd ones; -1 where the instant has no active slot.  beta = 1.25 throughout."""
    def make():
        pats = fit_patterns(K)
        rows = [pattern_row(K, pats[i % len(pats)], seed=31) for i in range(n)]
        edge, below = np.full(n, -1), np.full(n, -1)
        for i, (am, f) in enumerate(rows):
            act = np.flatnonzero((am != 0) & (f > 0))
            if len(act):
                s = act[-1]
                f[s] = AMP_F_EDGE if i % 2 == 0 else np.nextafter(AMP_F_EDGE, 0.0)
                (edge if i % 2 == 0 else below)[i] = s
        beta = np.full(n, AMP_BETA)
        assert AMP_BETA * AMP_F_EDGE == FS / 2 and AMP_BETA * np.nextafter(AMP_F_EDGE, 0.0) == np.nextafter(FS / 2, 0.0)
        return dict(rec=records_of(rows), beta=beta, edge=edge, below=below)
    return _once(("amp_case", n, K), make)


def amp_rows(n, P, a):
    """grid_rows of n instants, 9 at most (n = 4, 5, 9 have the empty rows of EMPTY_ROWS)."""
    return grid_rows(n, P, a)


def model_amplitudes(am, fm, fs, beta, C, a, alpha, warp, dtype=np.float64):
    if a is None:
        return CR.amplitudes(am, fm, fs, beta, C, alpha, warp, dtype)
    n = am.shape[0]
    bf = np.broadcast_to(np.asarray(beta, dtype=np.float64), (n,))[:, None] * fm
    active = (am != 0) & (fm > 0)
    with np.errstate(invalid="ignore"):     # cepstrum_warp_ref.amplitudes, with its readout in `dtype`
        A = np.exp(CW.readout(C, fs, CR.read_frequency(np.where(active, bf, 0.0), n, alpha, warp), a, dtype))
    return np.where(active & (bf < fs / 2), A, dtype(0))


def rel_error(got, ref):
    """max |got / ref - 1| over the cells where ref != 0; inf if the zero cells of the two differ."""
    got, ref = np.asarray(got), np.asarray(ref)
    if not np.array_equal(got == 0, ref == 0):
        return np.inf
    nz = ref != 0
    return float(np.abs(got[nz] / ref[nz] - 1).max()) if nz.any() else 0.0


def amp_models(n, K, P, a, mode):
    """dict(amp, amp_l, zero, dev): dev relative, over the cells that are not zero."""
    def make():
        c = amp_case(n, K)
        rec = c["rec"]
        C = amp_rows(n, P, a)
        alpha, warp = grid_mode(mode, n)
        args = (rec[:, :K], rec[:, K:2 * K], FS, c["beta"], C, a, alpha, warp)
        amp, amp_l = model_amplitudes(*args), model_amplitudes(*args, np.longdouble)
        return dict(amp=amp, amp_l=amp_l, zero=amp == 0, dev=rel_error(amp_l, amp))
    return _once(("amp", n, K, P, a, mode), make)


# ---- 6. the model build
BUILD_N = [2, 3, 4, 5, 9]
BUILD_K = [1, 63, 64, 65, 129]
BUILD_P = [2, 63]
KCAP = 1706
INSTANTS = ["normal", "nyquist", "unvoiced", "theta0", "empty", "underflow", "theta_top", "normal", "normal"]
THETA_TOP = 1.0 - 2.0 ** -53      # the largest float64 below 1


def build_fs(Kmax):
    return 48000.0 if Kmax == 129 else FS


def build_case(n, Kmax):
    """dict(fs, f0, theta, voiced, a0, edge_h): the first n of INSTANTS.  f0 is near 120 Hz (16 kHz: 66 harmonics below
    fs/2, so every slot up to Kmax = 65 is active) or near 180 Hz (48 kHz, Kmax = 129: 133 harmonics); the nyquist
    instant has h f0 == fs/2 exactly at h = edge_h: f0 = 1000 Hz and h = 8 at 16 kHz, 187.5 Hz and h = 128 at 48 kHz,
    and f0 = fs/2 itself, h = 1, at Kmax = 1.  theta is random in [0, 1) but 0 at theta0 and 1 - 2^-53 at theta_top."""
    fs = build_fs(Kmax)
    rng = np.random.default_rng([n, Kmax])
    base = 180.0 if Kmax == 129 else 120.0
    f0 = base + rng.uniform(-2.0, 2.0, n)
    theta = rng.uniform(0.0, 1.0, n)
    voiced = np.ones(n, dtype=bool)
    edge_h = 1 if Kmax == 1 else 128 if Kmax == 129 else 8
    for i, kind in enumerate(INSTANTS[:n]):
        if kind == "nyquist":
            f0[i] = fs / 2 / edge_h
        elif kind == "unvoiced":
            voiced[i] = False
        elif kind == "theta0":
            theta[i] = 0.0
        elif kind == "theta_top":
            theta[i] = THETA_TOP
    assert np.float64(edge_h) * f0[1] == fs / 2 and edge_h <= max(Kmax, 1)
    return dict(fs=fs, f0=f0, theta=theta, voiced=voiced, a0=0.01 * (1 + np.arange(n)) * (-1.0) ** np.arange(n),
                edge_h=edge_h)


def build_rows(n, Kmax, P, a):
    """Rows fitted by the model (lam = 5e-4, axis a) to n instants of harmonics of 190 Hz up to fs/2; the `empty`
    instant's row is (-inf, 0, .., 0) and the `underflow` instant's has c_0 = -800."""
    def make():
        fs = build_fs(Kmax)
        f = 190.0 * np.arange(1, int(fs / 2 / 190.0))
        rows = [(np.exp(ln_am(f, 40.0 * i)), f) if INSTANTS[i] != "empty" else (np.zeros(len(f)), f) for i in range(n)]
        C = model_fit(records_of(rows), fs, P, 5e-4, a)
        for i, kind in enumerate(INSTANTS[:n]):
            if kind == "underflow":
                C[i, 0] = -800.0
        return C
    return _once(("build_rows", n, Kmax, P, a), make)


def model_build(case, C, Kmax, Kcap, zero_phase, a, dtype=np.float64):
    """The records of eaqhm_model_build from (f0, theta, voiced, rows): model_build_ref.build's cell arithmetic with
    theta given, not integrated.  dict(am, fm, ph [n, Kmax] in `dtype` (fm float64), active)."""
    fs, f0, th, voiced = case["fs"], case["f0"], case["theta"], case["voiced"]
    n = len(f0)
    has = voiced & ~np.isneginf(C[:, 0])
    h = np.arange(1, Kmax + 1, dtype=np.float64)
    fm = h[None, :] * f0[:, None]                                    # the float64 product
    live = has[:, None] & (fm < fs / 2) & (np.arange(Kmax)[None, :] < Kcap)
    Cs = np.where(has[:, None], C, 0.0)
    with np.errstate(over="ignore", under="ignore"):
        lnam, phi = MB.series(Cs, fs, fm, dtype) if a is None else CW.series(Cs, fs, fm, a, dtype)
        am = np.exp(lnam)
    if zero_phase:
        phi = np.zeros_like(phi)
    active = live & (am.astype(np.float64) != 0)
    ht = h.astype(dtype)[None, :] * th.astype(dtype)[:, None]
    ph = MB.wrap((2 * CR._pi(dtype)) * (ht - np.floor(ht)) + phi)
    z = dtype(0)
    return dict(am=np.where(active, am, z), fm=np.where(active, fm, 0.0), ph=np.where(active, ph, z), active=active)


def build_models(n, Kmax, P, a, zero_phase):
    """dict(m, m_l, dev_am (relative, over the active cells), dev_ph (wrapped)) at Kcap = Kmax."""
    def make():
        case, C = build_case(n, Kmax), build_rows(n, Kmax, P, a)
        m = model_build(case, C, Kmax, Kmax, zero_phase, a)
        m_l = model_build(case, C, Kmax, Kmax, zero_phase, a, np.longdouble)
        assert np.array_equal(m["active"], m_l["active"])
        return dict(m=m, m_l=m_l, dev_am=rel_error(m_l["am"], m["am"]),
                    dev_ph=float(np.abs(wrapped(m["ph"] - m_l["ph"])).max()))
    return _once(("build", n, Kmax, P, a, bool(zero_phase)), make)
