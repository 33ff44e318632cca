"""The discrete-cepstrum envelope, a harmonic model built from f0 and cepstral rows (§9.7) and the
all-pass warped frequency axis (§9.8).  The fits, readouts and the build run in libeaqhm_hip.so (eaqhm_model_cepstrum,
eaqhm_cepstrum_envelope, eaqhm_cepstrum_phase, eaqhm_model_build and their *_warped siblings); there is no CPU path.

    model_cepstrum(DetComponents, fs, order=None, lam=5e-4, *, cep_warp=0.0, device_index=0) -> float64[No_ti, order + 1]
    check_model_cepstrum_arguments(model, fs, order=None, lam=5e-4)
    cepstrum_envelope(ceps, fs, freqs, formant_scale=1.0, formant_warp=None, *, cep_warp=0.0, device_index=0)
        -> float64[n, len(freqs)]
    cepstrum_phase(ceps, fs, freqs, formant_scale=1.0, formant_warp=None, *, cep_warp=0.0, device_index=0)
        -> float64[n, len(freqs)]
    check_envelope_cepstrum(model, envelope, preserve_envelope) -> float64[No_ti, P + 1]
    model_parameters(DetComponents, fs, order=None, lam=5e-4, *, cep_warp=0.0, device_index=0)
        -> dict(f0, ceps, voiced, step, fs), and cep_warp when it is not 0
    model_from_parameters(f0, ceps, fs, step, *, voiced=None, phase="minimum", theta0=0.0, kmax=None, a0=None,
                          cep_warp=0.0, device_index=0) -> det_format="arrays" dict (ti, isVoiced, a0, amplitudes, frange, pk)
    check_model_build_arguments(f0, ceps, fs, step, voiced=None, phase="minimum", theta0=0.0, kmax=None, a0=None)
    harmonic_counts(f0, fs, cap) -> int64[n]; fundamental_phase(g, theta0, step, fs) -> float64[n] in [0, 1)
    check_cepstrum_warp(cep_warp, name="cep_warp") -> float, |a| <= 0.9
    allpass_warp(a, w) -> Omega_a(w); cepstrum_warp(fs, scale="mel") -> the coefficient of a perceptual scale
    rewarp_matrix(b, order_in, order_out) -> float64[order_out + 1, order_in + 1]
    cepstrum_rewarp(ceps, cep_warp_in, cep_warp_out, order=None) -> the rows on the other axis
    check_cepstrum_rewarp_arguments(ceps, cep_warp_in, cep_warp_out, order=None)

Constants: CEPSTRUM_MAX_ORDER, CEPSTRUM_LAMBDA_RANGE, CEPSTRUM_WARP_MAX, CEPSTRUM_WARP_SCALES, BUILD_MAX_HARMONICS,
BUILD_PHASES.
"""
from functools import partial

import numpy as np

from .args import _contour, _freq_grid, _integer, _numeric_1d, _sample_rate, _warp_excludes_scale, _warp_rows
from .records import _device, _device_records, model_f0, unpack_model


# ---- the discrete-cepstrum envelope
CEPSTRUM_MAX_ORDER = 63          # lane r of a wave owns row r of the (order + 1)-square system
CEPSTRUM_LAMBDA_RANGE = (1e-6, 1.0)


CEPSTRUM_WARP_MAX = 0.9          # |cep_warp| at most: the fit and the readouts are checked up to it
CEPSTRUM_WARP_SCALES = ("mel", "bark")


def check_cepstrum_warp(cep_warp, name="cep_warp"):
    """Validates the coefficient of the all-pass warped axis (no device work): a finite number with
    |a| <= 0.9; 0 is the linear axis.  Returns it as a float."""
    if isinstance(cep_warp, (bool, np.bool_)) or not isinstance(cep_warp, (int, float, np.integer, np.floating)):
        raise ValueError("%s must be a number in [-%g, %g], got %r" % (name, CEPSTRUM_WARP_MAX, CEPSTRUM_WARP_MAX,
                                                                       cep_warp))
    a = float(cep_warp)
    if not abs(a) <= CEPSTRUM_WARP_MAX:                # also rejects NaN
        raise ValueError("%s must be finite and in [-%g, %g], got %r" % (name, CEPSTRUM_WARP_MAX, CEPSTRUM_WARP_MAX, a))
    return a


def _on_axis(c, method, a):
    """The Context method `method` on the axis a: the method itself at a == 0 (the calls are then exactly those made
    without a warped axis), else its *_warped sibling with cep_warp bound."""
    if a == 0.0:
        return getattr(c, method)
    return partial(getattr(c, method + "_warped"), cep_warp=a)


def _cepstrum_order(order):
    order = _integer(order, "order")
    if not 1 <= order <= CEPSTRUM_MAX_ORDER:
        raise ValueError("order must be in [1, %d], got %d" % (CEPSTRUM_MAX_ORDER, order))
    return order


def _cepstrum_lambda(lam):
    try:
        lam = float(lam)
    except (TypeError, ValueError):
        raise ValueError("lam must be a number") from None
    if not CEPSTRUM_LAMBDA_RANGE[0] <= lam <= CEPSTRUM_LAMBDA_RANGE[1]:     # also rejects NaN
        raise ValueError("lam must be in [%g, %g], got %r" % (CEPSTRUM_LAMBDA_RANGE + (lam,)))
    return lam


def check_model_cepstrum_arguments(model, fs, order=None, lam=5e-4):
    """Validates everything model_cepstrum gets but cep_warp, which is check_cepstrum_warp's (no device work): returns
    (fs, order, lam).  order defaults to min(63, 2 + round(fs / 1000)), the LPC order of eaQHMNoiseAnalysis; lam must be
    in [1e-6, 1]."""
    fs = _sample_rate(fs)
    order = min(CEPSTRUM_MAX_ORDER, 2 + int(round(fs / 1000.0))) if order is None else _cepstrum_order(order)
    lam = _cepstrum_lambda(lam)
    rec = model["records"]
    if not np.all(np.isfinite(rec)):
        raise ValueError("the model holds non-finite values")
    if np.any(rec[:, :model["Kmax"]] < 0):
        raise ValueError("amplitudes must be >= 0 (the model holds |a_k|)")
    return fs, order, lam


def model_cepstrum(DetComponents, fs, order=None, lam=5e-4, *, cep_warp=0.0, device_index=0):
    """The discrete cepstrum of every analysis instant: order + 1 coefficients of the smooth
    log-amplitude envelope C(w) = c_0 + 2 sum_p c_p cos(p w), w = 2 pi f / fs, fitted to the instant's active partials
    (w_n, ln |a_n|) by least squares with the penalty lam * sum_p 8 pi^2 p^2 c_p^2 (c_0 is free).  An instant with fewer
    partials than coefficients is fitted like any other; one without any gives the row (-inf, 0, .., 0).  `order`
    defaults to min(63, 2 + round(fs / 1000)), `lam` lies in [1e-6, 1].  The rows are plain arrays: they can be smoothed
    over time, blended with another model's, and passed to eaQHMSynthesis(envelope=) and cepstrum_envelope.  Raises
    numpy.linalg.LinAlgError when the factorisation of an instant broke down.

    `cep_warp` = a, |a| <= 0.9, fits on the all-pass warped axis instead (§9.8): C(w) = c_0 + 2 sum_p c_p cos(p
    Omega_a(w)), Omega_a(w) = w + 2 atan2(a sin w, 1 - a cos w), with the nodes at Omega_a(w_n) and the penalty as
    smoothness on that axis.  a > 0 spends the order where speech has structure: cepstrum_warp(fs) gives the a that
    follows the mel scale.  The rows keep their layout, and nothing in them says which axis they lie on: every
    function that reads them at a frequency (cepstrum_envelope, cepstrum_phase, eaQHMSynthesis, model_from_parameters,
    noise_from_cepstrum) must be given the same cep_warp, and rows of different axes must not be aligned, paired or
    blended with each other (cepstrum_rewarp moves rows between axes).  0, the default, is the linear axis.

    Returns float64[No_ti, order + 1]."""
    model = unpack_model(DetComponents)
    fs, order, lam = check_model_cepstrum_arguments(model, fs, order, lam)
    axis = check_cepstrum_warp(cep_warp)
    torch, c, dev = _device(device_index)
    rec, n, K = _device_records(model, dev)
    ceps = torch.empty((n, order + 1), dtype=torch.float64, device=dev)
    _on_axis(c, "model_cepstrum", axis)(rec, n, K, fs, order, lam, ceps)
    out = ceps.cpu().numpy()
    bad = np.flatnonzero(np.isnan(out).any(axis=1))
    if len(bad):
        raise np.linalg.LinAlgError("the cepstral fit of %d instant(s) broke down (the first: %d)" % (len(bad), bad[0]))
    return out


def _cepstrum_rows(ceps, name, rows=None):
    """A cepstrum as contiguous float64[n, P + 1], validated: 1 <= P <= 63, every entry finite except that a row may be
    (-inf, 0, .., 0), the empty envelope."""
    C = np.asarray(ceps)
    if C.dtype.kind not in "iuf" or C.ndim != 2:
        raise ValueError("%s must be a 2-D array of numbers, one row of order + 1 coefficients per instant" % name)
    if rows is not None and C.shape[0] != rows:
        raise ValueError("%s must have one row per analysis instant (%d), got %d" % (name, rows, C.shape[0]))
    if C.shape[0] < 1 or not 1 <= C.shape[1] - 1 <= CEPSTRUM_MAX_ORDER:
        raise ValueError("%s must have at least one row and 2 to %d columns (order 1 to %d), got shape %s"
                         % (name, CEPSTRUM_MAX_ORDER + 1, CEPSTRUM_MAX_ORDER, C.shape))
    C = np.ascontiguousarray(C, dtype=np.float64)
    empty = np.isneginf(C[:, 0]) & np.all(C[:, 1:] == 0, axis=1)
    if not np.all(np.isfinite(C[~empty])):
        raise ValueError("%s must be finite; only a whole row may be (-inf, 0, .., 0), the empty envelope" % name)
    return C


def check_envelope_cepstrum(model, envelope, preserve_envelope):
    """Validates eaQHMSynthesis's `envelope` (no device work): float64[No_ti, P + 1], 1 <= P <= 63, finite except for
    rows (-inf, 0, .., 0); it needs preserve_envelope=True.  Returns it contiguous."""
    if not preserve_envelope:
        raise ValueError("envelope= needs preserve_envelope=True: without it each partial keeps its own amplitude")
    return _cepstrum_rows(envelope, "envelope", len(model["ti"]))


def cepstrum_envelope(ceps, fs, freqs, formant_scale=1.0, formant_warp=None, *, cep_warp=0.0, device_index=0):
    """The envelope a cepstrum describes, on a frequency grid: out[i, t] = C_i(freqs[t] / alpha_i), the
    natural log of the amplitude, with C_i(q) = c_0 + 2 sum_p c_p cos(2 pi p q^ / fs), q^ = min(max(q, 0), fs/2) (held
    past Nyquist).  `ceps` is float64[n, P + 1] (model_cepstrum's, or any blend of such); a row (-inf, 0, .., 0) reads
    -inf.  `formant_scale` = alpha is a number or one value per row, in [0.25, 4]; `formant_warp` = (f_in, f_out) reads
    C_i(W_i^-1(freqs[t])) instead (f_out [B] or one row per row of `ceps`) and excludes a formant_scale != 1.  It is the
    envelope eaQHMSynthesis(envelope=ceps) reads at that scale or map.  With `cep_warp` = a, |a| <= 0.9, the rows lie on
    the all-pass warped axis of §9.8: the read frequency is formed in Hz as above, held, and then warped,
    C_i(q) = c_0 + 2 sum_p c_p cos(p Omega_a(2 pi q^ / fs)).  Returns float64[n, len(freqs)]."""
    fs = _sample_rate(fs)
    C = _cepstrum_rows(ceps, "ceps")
    f = _freq_grid(freqs)
    axis = check_cepstrum_warp(cep_warp)
    n, P = C.shape[0], C.shape[1] - 1
    alpha = _contour(formant_scale, "formant_scale", n)
    wmap = None
    if formant_warp is not None:
        _warp_excludes_scale(formant_scale)
        wmap = _warp_rows(formant_warp, n, "row of ceps")
    torch, c, dev = _device(device_index)
    C_d, f_d = torch.as_tensor(C, device=dev), torch.as_tensor(np.ascontiguousarray(f), device=dev)
    out = torch.empty((n, len(f)), dtype=torch.float64, device=dev)
    read = _on_axis(c, "cepstrum_envelope", axis)
    if wmap is not None:
        x_d, y_d = (torch.as_tensor(np.array(v), device=dev) for v in wmap)      # a broadcast row is read-only: a copy
        read(C_d, n, P, fs, f_d, len(f), out, warp=(x_d, y_d, len(wmap[0])))
    elif np.any(alpha != 1.0):
        read(C_d, n, P, fs, f_d, len(f), out, alpha=torch.as_tensor(alpha, device=dev))
    else:
        read(C_d, n, P, fs, f_d, len(f), out)
    return out.cpu().numpy()


# ---- a harmonic model from f0 and cepstral rows
BUILD_MAX_HARMONICS = 1706       # Kmax of a model at most: the LDS limit of eaqhm_modify_prep
BUILD_PHASES = ("minimum", "zero")


def harmonic_counts(f0, fs, cap):
    """Per instant the number of harmonics h = 1, 2, .. with h * f0 < fs / 2 in float64 (this product against this
    half: the comparison eaqhm_model_build makes), at most `cap`; 0 where f0 is not > 0.  int64[n]."""
    f0 = np.asarray(f0, dtype=np.float64)
    half = 0.5 * float(fs)
    ok = f0 > 0
    g = np.where(ok, f0, 1.0)
    m = np.minimum(np.floor(half / g), float(cap))
    for _ in range(4):           # the quotient is off by one at the most; the product decides
        m = np.where(((m + 1.0) * g < half) & (m + 1.0 <= cap), m + 1.0, m)
        m = np.where((m >= 1.0) & (m * g >= half), m - 1.0, m)
    return np.where(ok, m, 0.0).astype(np.int64)


def fundamental_phase(g, theta0, step, fs):
    """theta of DESIGN.md §9.7: the fundamental's phase in cycles at every instant, theta_0 = theta0,
    theta_{i+1} = frac(theta_i + (step / fs) (g_i + g_{i+1}) / 2), in float64 in this order (fundamental_advance's, with
    the whole frequency in place of the excess)."""
    g = np.asarray(g, dtype=np.float64)
    inc = (float(step) / float(fs)) * (g[:-1] + g[1:]) / 2
    th = np.zeros(len(g))
    acc = th[0] = float(theta0)
    for j, d in enumerate(inc.tolist()):
        acc += d
        acc -= np.floor(acc)
        th[j + 1] = acc
    return th


def _held(x, has):
    """x where `has`, elsewhere the value of the nearest earlier instant that has one, else of the nearest later one
    (the rule of _records_f0); zeros when none has."""
    n = len(x)
    if not has.any():
        return np.zeros(n)
    src = np.maximum.accumulate(np.where(has, np.arange(n), -1))
    src[src < 0] = int(np.flatnonzero(has)[0])
    return np.where(has, x, 0.0)[src]


def check_model_build_arguments(f0, ceps, fs, step, voiced=None, phase="minimum", theta0=0.0, kmax=None, a0=None):
    """Validates everything model_from_parameters gets and prepares what the host owes the kernel (no device work).
    Returns dict(f0, ceps, fs, step, voiced, zero_phase, a0, theta, counts, Kmax, Kcap): f0 with zeros at unvoiced
    instants, theta the fundamental's phase in cycles, counts the harmonics below fs/2 per instant (0 at an unvoiced
    instant or an empty row), Kmax = max(1, counts.max()).  (cep_warp is check_cepstrum_warp's.)"""
    fs = _sample_rate(fs)
    step = _integer(step, "step")
    if step <= 0:
        raise ValueError("step must be a positive integer (samples), got %d" % step)
    f = np.asarray(f0)
    if f.dtype.kind not in "iuf" or f.ndim != 1:
        raise ValueError("f0 must be a 1-D array of numbers (Hz), one per analysis instant")
    f = f.astype(np.float64)
    n = len(f)
    if n < 2:
        raise ValueError("the model needs at least two analysis instants")
    if voiced is None:
        with np.errstate(invalid="ignore"):
            v = f > 0
    else:
        v = np.asarray(voiced)
        if v.dtype.kind not in "biu" or v.shape != (n,):
            raise ValueError("voiced must be a 1-D array of booleans, one per analysis instant (%d)" % n)
        v = v.astype(bool)
    if not v.any():
        raise ValueError("no voiced instant: there is nothing to build")
    fv = f[v]
    if not np.all(np.isfinite(fv)) or np.any(fv <= 0) or np.any(fv >= 0.5 * fs):
        raise ValueError("f0 of a voiced instant must be finite and in (0, fs/2) Hz")
    C = _cepstrum_rows(ceps, "ceps", n)
    if phase not in BUILD_PHASES:
        raise ValueError("phase must be one of %s, got %r" % (", ".join(map(repr, BUILD_PHASES)), phase))
    try:
        theta0 = float(theta0)
    except (TypeError, ValueError):
        raise ValueError("theta0 must be a number (cycles)") from None
    if not np.isfinite(theta0):
        raise ValueError("theta0 must be finite (cycles)")
    Kcap = BUILD_MAX_HARMONICS
    if kmax is not None:
        Kcap = _integer(kmax, "kmax")
        if not 1 <= Kcap <= BUILD_MAX_HARMONICS:
            raise ValueError("kmax must be in [1, %d], got %d" % (BUILD_MAX_HARMONICS, Kcap))
    if a0 is None:
        a = np.zeros(n)
    else:
        a = _numeric_1d(a0, "a0")
        if len(a) != n or not np.all(np.isfinite(a)):
            raise ValueError("a0 must hold one finite value per analysis instant (%d)" % n)
    has = v & ~np.isneginf(C[:, 0])
    f = np.where(v, f, 0.0)
    counts = harmonic_counts(np.where(has, f, 0.0), fs, Kcap)
    theta = fundamental_phase(_held(f, has), theta0, step, fs)
    return dict(f0=f, ceps=C, fs=fs, step=step, voiced=v, zero_phase=phase == "zero", a0=a, theta=theta, counts=counts,
                Kmax=max(1, int(counts.max())), Kcap=Kcap)


def model_from_parameters(f0, ceps, fs, step, *, voiced=None, phase="minimum", theta0=0.0, kmax=None, a0=None,
                          cep_warp=0.0, device_index=0):
    """A harmonic model from a fundamental track and a cepstral envelope, the inverse of
    model_parameters: per analysis instant i (at sample i * step) `f0[i]` in Hz, `voiced[i]` (default f0 > 0) and the
    row `ceps[i]` of model_cepstrum's layout, from this or another model or from a pipeline of the caller's own.  Slot k
    holds harmonic h = k + 1 at h f0 with the amplitude exp(C_i(h f0)) and the phase 2 pi frac(h theta_i) + Phi_i(h f0),
    wrapped; theta is the running phase of the fundamental in cycles from `theta0`, with f0 held across unvoiced
    instants, and Phi the minimum-phase response of the envelope, -2 sum_p c_p sin(2 pi p f / fs) (phase="zero": 0,
    pulse-like harmonics).  A slot is active while the instant is voiced, its row is not (-inf, 0, .., 0), h f0 < fs/2
    and k < kmax (default and limit 1706).  `a0` is the DC term per instant (default 0; unpack_model drops it at
    unvoiced instants, as for an analysed model).  `cep_warp` = a, |a| <= 0.9, reads rows that lie on the all-pass
    warped axis (§9.8; model_parameters(cep_warp=a) gives such): C and Phi at Omega_a(2 pi h f0 / fs).

    Returns the model as a det_format="arrays" dict (ti, isVoiced, a0, amplitudes, frange, pk), which unpack_model,
    eaQHMSynthesis and every other function here take like an analysed one.  The records take n * (3 Kmax + 1) * 8
    bytes on the device and on the host."""
    a = check_model_build_arguments(f0, ceps, fs, step, voiced, phase, theta0, kmax, a0)
    axis = check_cepstrum_warp(cep_warp)
    torch, c, dev = _device(device_index)
    n, K, C = len(a["f0"]), a["Kmax"], a["ceps"]
    f_d, th_d, a0_d, C_d = (torch.as_tensor(np.ascontiguousarray(x), device=dev)
                            for x in (a["f0"], a["theta"], a["a0"], C))
    v_d = torch.as_tensor(a["voiced"].astype(np.uint8), device=dev)
    rec = torch.empty((n, 3 * K + 1), dtype=torch.float64, device=dev)
    _on_axis(c, "model_build", axis)(f_d, th_d, v_d, C_d, C.shape[1] - 1, a0_d, n, a["fs"], K, a["Kcap"],
                                     a["zero_phase"], rec)
    r = rec.cpu().numpy()
    return dict(ti=np.arange(n, dtype=np.int64) * a["step"], isVoiced=a["voiced"].copy(), a0=r[:, 3 * K].copy(),
                amplitudes=r[:, :K].copy(), frange=r[:, K:2 * K].copy(), pk=r[:, 2 * K:3 * K].copy())


def cepstrum_phase(ceps, fs, freqs, formant_scale=1.0, formant_warp=None, *, cep_warp=0.0, device_index=0):
    """The minimum-phase response of the envelope a cepstrum describes, on a frequency grid:
    out[i, t] = Phi_i(freqs[t] / alpha_i), Phi_i(q) = -2 sum_p c_p sin(2 pi p q^ / fs) at cepstrum_envelope's read
    frequency q^, in radians as the series gives it (not wrapped).  exp(C + j Phi) is the frequency response of the
    causal, minimum-phase filter whose log magnitude is C.  The arguments are cepstrum_envelope's; a row
    (-inf, 0, .., 0) reads 0.  With `cep_warp` = a the rows lie on the warped axis of §9.8 and
    Phi_i(q) = -2 sum_p c_p sin(p Omega_a(2 pi q^ / fs)): the all-pass substitution maps the unit disc onto itself, so it
    is still the minimum-phase response of the envelope the rows describe.  Returns float64[n, len(freqs)]."""
    fs = _sample_rate(fs)
    C = _cepstrum_rows(ceps, "ceps")
    f = _freq_grid(freqs)
    axis = check_cepstrum_warp(cep_warp)
    n, P = C.shape[0], C.shape[1] - 1
    alpha = _contour(formant_scale, "formant_scale", n)
    wmap = None
    if formant_warp is not None:
        _warp_excludes_scale(formant_scale)
        wmap = _warp_rows(formant_warp, n, "row of ceps")
    torch, c, dev = _device(device_index)
    C_d, f_d = torch.as_tensor(C, device=dev), torch.as_tensor(np.ascontiguousarray(f), device=dev)
    out = torch.empty((n, len(f)), dtype=torch.float64, device=dev)
    read = _on_axis(c, "cepstrum_phase", axis)
    if wmap is not None:
        x_d, y_d = (torch.as_tensor(np.array(v), device=dev) for v in wmap)      # a broadcast row is read-only: a copy
        read(C_d, n, P, fs, f_d, len(f), out, warp=(x_d, y_d, len(wmap[0])))
    elif np.any(alpha != 1.0):
        read(C_d, n, P, fs, f_d, len(f), out, alpha=torch.as_tensor(alpha, device=dev))
    else:
        read(C_d, n, P, fs, f_d, len(f), out)
    return out.cpu().numpy() + 0.0        # the -0.0 of an empty row reads 0.0


def model_parameters(DetComponents, fs, order=None, lam=5e-4, *, cep_warp=0.0, device_index=0):
    """The model reduced to plain arrays: dict(f0=model_f0(..), ceps=model_cepstrum(..), voiced, step,
    fs), `voiced` being "the instant has an active slot".  Each entry can be edited, smoothed, predicted or taken from
    another model; model_from_parameters(p["f0"], p["ceps"], p["fs"], p["step"], voiced=p["voiced"]) is the way back.
    With `cep_warp` = a != 0 the rows are model_cepstrum(cep_warp=a)'s (§9.8) and the dict also holds cep_warp=a, which
    the way back needs as model_from_parameters(..., cep_warp=p["cep_warp"])."""
    axis = check_cepstrum_warp(cep_warp)
    model = unpack_model(DetComponents)
    K = model["Kmax"]
    voiced = (model["records"][:, :K] != 0).any(axis=1)
    extra = dict(cep_warp=axis) if axis != 0.0 else {}
    return dict(f0=model_f0(DetComponents, fs),
                ceps=model_cepstrum(DetComponents, fs, order, lam, device_index=device_index, **extra),
                voiced=voiced, step=model["step"], fs=_sample_rate(fs), **extra)


# ---- the warped axis on the host
def allpass_warp(a, w):
    """Omega_a(w) = w + 2 atan2(a sin w, 1 - a cos w): the phase of the all-pass (z^-1 - a) / (1 - a z^-1), strictly
    increasing on [0, pi] with Omega_a(0) = 0, Omega_a(pi) = pi and Omega_a^-1 = Omega_{-a}.  Works in the dtype of w."""
    return w + 2 * np.arctan2(a * np.sin(w), 1 - a * np.cos(w))


def cepstrum_warp(fs, scale="mel"):
    """A coefficient for `cep_warp` that makes the all-pass warped axis follow a perceptual scale at the
    sampling rate `fs`.  "mel": the a in [0, 0.9] that minimises sum_{t=0..512} (Omega_a(pi t / 512) - pi mel(f_t) /
    mel(fs / 2))^2 with f_t = t fs / 1024 and mel(f) = 2595 log10(1 + f / 700), to 1e-6: 0.3624 at 8 kHz, 0.4595 at
    16 kHz, 0.5019 at 22.05 kHz, 0.5853 at 44.1 kHz, 0.5946 at 48 kHz.  "bark": Smith & Abel's (1999) closed form
    1.0674 sqrt((2 / pi) atan(0.06583 fs / 1000)) - 0.1916, 0.5755 at 16 kHz and 0.7564 at 44.1 kHz.  The customary table
    value 0.42 at 16 kHz is the optimum of another criterion (another mel formula and error measure); any number in
    [-0.9, 0.9] is the caller's choice, and what matters is that fit and readouts use the same one.  Host only."""
    fs = _sample_rate(fs)
    if scale == "bark":
        return check_cepstrum_warp(1.0674 * np.sqrt((2.0 / np.pi) * np.arctan(0.06583 * fs / 1000.0)) - 0.1916,
                                   "the Bark coefficient at this fs")
    if scale != "mel":
        raise ValueError("scale must be one of %s, got %r" % (", ".join(map(repr, CEPSTRUM_WARP_SCALES)), scale))
    t = np.arange(513)
    w = np.pi * t / 512.0
    mel = np.log10(1.0 + (t * fs / 1024.0) / 700.0)
    target = np.pi * mel / mel[-1]

    def cost(a):
        return float(((allpass_warp(a, w) - target) ** 2).sum())

    grid = np.linspace(0.0, CEPSTRUM_WARP_MAX, 91)
    j = int(np.argmin([cost(a) for a in grid]))
    lo, hi = grid[max(j - 1, 0)], grid[min(j + 1, 90)]
    g = (np.sqrt(5.0) - 1.0) / 2.0                     # golden section within the bracket of the grid's minimum
    x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
    c1, c2 = cost(x1), cost(x2)
    while hi - lo > 1e-7:
        if c1 <= c2:
            hi, x2, c2 = x2, x1, c1
            x1 = hi - g * (hi - lo)
            c1 = cost(x1)
        else:
            lo, x1, c1 = x1, x2, c2
            x2 = lo + g * (hi - lo)
            c2 = cost(x2)
    return float(0.5 * (lo + hi))


def rewarp_matrix(b, order_in, order_out):
    """A float64[order_out + 1, order_in + 1] with c~ = A c: the rows c of C(w) = c_0 + 2 sum_p c_p cos(p w') on one
    axis w' to the rows c~ of the same function on the axis Omega_b(w').  In the conventional cepstrum
    k_0 = c_0, k_p = 2 c_p it is Oppenheim & Johnson's frequency transformation, built column by column by its
    recursion (the one SPTK calls freqt) in np.longdouble and rounded once."""
    ld = np.longdouble
    b = ld(b)
    g = np.zeros((order_out + 1, order_in + 1), dtype=ld)
    unit = np.eye(order_in + 1, dtype=ld)
    for i in range(order_in, -1, -1):              # every column of the map at once: the input is the unit matrix
        d = g.copy()
        g[0] = unit[i] + b * d[0]
        g[1] = (1 - b * b) * d[0] + b * d[1]
        for j in range(2, order_out + 1):
            g[j] = d[j - 1] + b * (d[j] - g[j - 1])
    k_in, k_out = np.full(order_in + 1, 2, dtype=ld), np.full(order_out + 1, 2, dtype=ld)
    k_in[0] = k_out[0] = 1
    return ((g * k_in[None, :]) / k_out[:, None]).astype(np.float64)


def check_cepstrum_rewarp_arguments(ceps, cep_warp_in, cep_warp_out, order=None):
    """Validates everything cepstrum_rewarp gets: returns (rows float64[n, P + 1], b, order) with b = (a_out - a_in) /
    (1 - a_in a_out), the coefficient of the composed all-pass, which must itself lie in [-0.9, 0.9]."""
    C = _cepstrum_rows(ceps, "ceps")
    a_in, a_out = check_cepstrum_warp(cep_warp_in, "cep_warp_in"), check_cepstrum_warp(cep_warp_out, "cep_warp_out")
    order = C.shape[1] - 1 if order is None else _cepstrum_order(order)
    b = (a_out - a_in) / (1.0 - a_in * a_out)
    if not abs(b) <= CEPSTRUM_WARP_MAX:
        raise ValueError("the composed warp (cep_warp_out - cep_warp_in) / (1 - cep_warp_in cep_warp_out) = %.4f must "
                         "lie in [-%g, %g]: move the rows in two steps" % (b, CEPSTRUM_WARP_MAX, CEPSTRUM_WARP_MAX))
    return C, b, order


def cepstrum_rewarp(ceps, cep_warp_in, cep_warp_out, order=None):
    """Moves cepstral rows from the axis `cep_warp_in` to the axis `cep_warp_out` (0 is the linear axis):
    the rows of the same envelope C(w) on the other axis, C @ A.T with A = rewarp_matrix(b, P, order), b the coefficient
    of the composed all-pass.  `order` (default: the input's) cuts or pads the result; cutting is the least-squares
    projection on the new axis, and the envelope moves by at most the tail 2 sum_{p > order} |c~_p|.  An empty row
    (-inf, 0, .., 0) comes back empty; equal warps and orders return the rows bit for bit.  This is how noise_cepstrum's
    rows, which are exact on the linear axis, reach the axis of a warped model: cepstrum_rewarp(rows, 0.0, a).  Host
    NumPy, like warp_rows.  Returns float64[n, order + 1]."""
    C, b, order = check_cepstrum_rewarp_arguments(ceps, cep_warp_in, cep_warp_out, order)
    if b == 0.0 and order == C.shape[1] - 1:
        return C.copy()
    empty = np.isneginf(C[:, 0])
    out = np.where(empty[:, None], 0.0, C) @ rewarp_matrix(b, C.shape[1] - 1, order).T
    out[empty, 0] = -np.inf
    return out
