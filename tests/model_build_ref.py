"""NumPy model of the harmonic model built from f0 and cepstral rows, written from the definition and
independently of the HIP kernel; the GPU tests compare eaqhm_model_build and eaqhm_cepstrum_phase with it.

Per instant i (at sample i * step): slot k holds harmonic h = k + 1.  It is active iff the instant is voiced, its row is
not (-inf, 0, .., 0), k < Kcap and h * f0_i < fs / 2 (the float64 product), and exp(C_i) did not underflow.  Then
    f = h f0_i,   |a| = exp(C_i(f)),   phase = wrap(2 pi frac(h theta_i) + Phi_i(f)),
    C_i(f) = c_0 + 2 sum_p c_p cos(p w),   Phi_i(f) = -2 sum_p c_p sin(p w),   w = 2 pi f / fs,
both sums from one Clenshaw recurrence (cosine sum b_1 cos w - b_2, sine sum b_1 sin w), the argument and the
recurrence in the order of model_cepstrum_ref.clenshaw; theta_0 = theta0, theta_{i+1} = frac(theta_i + (step / fs)
(g_i + g_{i+1}) / 2), g = f0 held over the instants that are unvoiced or empty.

    held(f0, has) -> g
    theta(g, theta0, step, fs, dtype) -> [n]
    series(ceps, fs, f, dtype) -> (C, Phi), each [n, F]; f is [F] or [n, F], read at min(max(f, 0), fs/2)
    wrap(x) -> x - 2 pi ceil((x - pi) / (2 pi)), in (-pi, pi]
    counts(f0, has, fs, Kcap) -> int[n]
    build(f0, voiced, ceps, fs, step, theta0=0, kmax=None, a0=None, zero_phase=False, dtype) -> dict(records, Kmax,
        active, lnam, carrier, phi): lnam = C at the active cells, carrier = 2 pi frac(h theta), phi = Phi (0 in zero
        phase), all [n, Kmax] in `dtype`; records float64[n, 3 Kmax + 1]

`dtype` selects the arithmetic (np.float64: the definition; np.longdouble: the yardstick the GPU tests take the phase
bar from).  The inputs, the active set and f = h f0 are float64 values in either case.
"""
import numpy as np

KCAP = 1706


def _pi(dtype):
    return dtype(np.pi) if dtype is np.float64 else np.arctan(dtype(1)) * 4


def held(f0, has):
    f0, has = np.asarray(f0, dtype=np.float64), np.asarray(has, dtype=bool)
    g = np.zeros(len(f0))
    if not has.any():
        return g
    first = int(np.flatnonzero(has)[0])
    last = f0[first]
    for i in range(len(f0)):
        if has[i]:
            last = f0[i]
        g[i] = last
    return g


def theta(g, theta0, step, fs, dtype=np.float64):
    g = np.asarray(g, dtype=np.float64).astype(dtype)
    th = np.zeros(len(g), dtype=dtype)
    acc = dtype(theta0)
    th[0] = acc
    for i in range(len(g) - 1):
        acc = acc + (dtype(step) / dtype(fs)) * (g[i] + g[i + 1]) / 2
        acc = acc - np.floor(acc)
        th[i + 1] = acc
    return th


def series(ceps, fs, f, dtype=np.float64):
    C = np.asarray(ceps, dtype=np.float64)
    n, P = C.shape[0], C.shape[1] - 1
    x = np.minimum(np.maximum(np.asarray(f, dtype=np.float64), 0.0), fs / 2)
    x = np.broadcast_to(x, (n, np.shape(f)[-1])).astype(dtype)
    Cd = C.astype(dtype)
    ang = ((2 * _pi(dtype)) * x) / dtype(fs)
    cs, sn = np.cos(ang), np.sin(ang)
    cw2 = 2 * cs
    b1, b2 = np.zeros(x.shape, dtype=dtype), np.zeros(x.shape, dtype=dtype)
    for p in range(P, 0, -1):
        b1, b2 = Cd[:, p, None] + (cw2 * b1 - b2), b1
    with np.errstate(invalid="ignore"):
        return 2 * (0.5 * cw2 * b1 - b2) + Cd[:, 0, None], -2 * (b1 * sn)


def wrap(x):
    dtype = x.dtype.type
    two_pi = 2 * _pi(dtype)
    return x - two_pi * np.ceil((x - _pi(dtype)) / two_pi)


def counts(f0, has, fs, Kcap=KCAP):
    """The number of h = 1.. with h * f0 < fs / 2 in float64, at most Kcap, by trying every h."""
    out = np.zeros(len(f0), dtype=np.int64)
    for i in np.flatnonzero(has):
        h = 1
        while h <= Kcap and np.float64(h) * np.float64(f0[i]) < np.float64(fs) / 2:
            h += 1
        out[i] = h - 1
    return out


def build(f0, voiced, ceps, fs, step, theta0=0.0, kmax=None, a0=None, zero_phase=False, dtype=np.float64):
    f0 = np.asarray(f0, dtype=np.float64)
    voiced = np.asarray(voiced, dtype=bool)
    C = np.asarray(ceps, dtype=np.float64)
    n = len(f0)
    has = voiced & ~np.isneginf(C[:, 0])
    Kcap = KCAP if kmax is None else int(kmax)
    cnt = counts(f0, has, fs, Kcap)
    K = max(1, int(cnt.max()))
    h = np.arange(1, K + 1, dtype=np.float64)
    f0z = np.where(has, f0, 0.0)
    fm = h[None, :] * f0z[:, None]                                    # the float64 product
    live = np.arange(K)[None, :] < cnt[:, None]
    assert np.array_equal(live, has[:, None] & (fm < fs / 2) & (np.arange(K)[None, :] < Kcap))
    Cs = np.where(has[:, None], C, 0.0)                               # an empty row is never read
    lnam, phi = series(Cs, fs, fm, dtype)
    if zero_phase:
        phi = np.zeros_like(phi)
    am = np.exp(lnam).astype(np.float64)
    active = live & (am != 0)
    th = theta(held(f0z, has), theta0, step, fs, dtype)
    ht = h.astype(dtype)[None, :] * th[:, None]
    carrier = (2 * _pi(dtype)) * (ht - np.floor(ht))
    ph = wrap(carrier + phi)
    rec = np.zeros((n, 3 * K + 1))
    rec[:, :K] = np.where(active, am, 0.0)
    rec[:, K:2 * K] = np.where(active, fm, 0.0)
    rec[:, 2 * K:3 * K] = np.where(active, ph.astype(np.float64), 0.0)
    rec[:, 3 * K] = 0.0 if a0 is None else np.asarray(a0, dtype=np.float64)
    return dict(records=rec, Kmax=K, active=active, lnam=lnam, carrier=carrier, phi=phi, phase=ph, theta=th,
                counts=cnt)


def det(rec, K, step, voiced):
    """The det_format="arrays" dict of records."""
    n = len(rec)
    return dict(ti=np.arange(n, dtype=np.int64) * step, isVoiced=np.asarray(voiced, dtype=bool).copy(),
                a0=rec[:, 3 * K].copy(), amplitudes=rec[:, :K].copy(), frange=rec[:, K:2 * K].copy(),
                pk=rec[:, 2 * K:3 * K].copy())
