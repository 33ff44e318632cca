"""Resynthesis from an analysed eaQHM model, with time and pitch scaling (not in the reference).

    unpack_model(DetComponents) -> dict(records, step, Kmax, ti, quirk_cells)
    eaQHMSynthesis(DetComponents, fs, length, time_scale=1.0, pitch_scale=1.0, preserve_envelope=True,
                   formant_scale=1.0, *, phase="independent", f0=None, formant_warp=None, envelope=None,
                   device_index=0) -> float64[L_out]
    model_cepstrum(DetComponents, fs, order=None, lam=5e-4, *, device_index=0) -> float64[No_ti, order + 1]
    cepstrum_envelope(ceps, fs, freqs, formant_scale=1.0, formant_warp=None, *, device_index=0) -> float64[n, len(freqs)]
    check_envelope_cepstrum(model, envelope, preserve_envelope) -> float64[No_ti, P + 1]
    model_align(CA, CB, band=None, c0_weight=0.0, empty_cost=4.0, *, device_index=0) -> (path int64[L, 2], cost)
    dtw(cost, band=None, *, device_index=0) -> (path int64[L, 2], total)
    alignment_index(path, nA) -> float64[nA]; warp_rows(X, idx) -> rows of X at fractional indices
    alignment_time_scale(path, nA, step_ratio=1.0) -> float64[nA]
    model_parameters(DetComponents, fs, order=None, lam=5e-4, *, device_index=0) -> dict(f0, ceps, voiced, step, fs)
    model_from_parameters(f0, ceps, fs, step, *, voiced=None, phase="minimum", theta0=0.0, kmax=None, a0=None,
                          device_index=0) -> det_format="arrays" dict (ti, isVoiced, a0, amplitudes, frange, pk)
    check_model_build_arguments(f0, ceps, fs, step, voiced=None, phase="minimum", theta0=0.0, kmax=None, a0=None)
    cepstrum_phase(ceps, fs, freqs, formant_scale=1.0, formant_warp=None, *, device_index=0) -> float64[n, len(freqs)]
    model_f0(DetComponents, fs) -> float64[No_ti]
    model_envelope(DetComponents, fs, freqs, formant_scale=1.0, formant_warp=None, *, device_index=0)
        -> float64[No_ti, len(freqs)]
    formant_warp_vtln(fs, alpha, knee=0.875) -> (f_in, f_out): the two-breakpoint VTLN map
    check_formant_warp(model, fs, formant_warp, formant_scale=1.0, preserve_envelope=True) -> (f_in[B], f_out[No_ti, B])
    noise_formant_warp(noise, DetComponents, formant_warp) -> (f_in[B], f_out[Nf, B])
    scale_contour(DetComponents, fs, times_s, values) -> float64[No_ti]
    contour_time_map(rho, beta, step, length) -> dict(rate, gain, C, L_out, rate_min)
    eaQHMNoiseAnalysis(s, s_recon, fs, order=None, hop=None, *, device_index=0) -> dict(sigma, refl, hop, order, fs, length)
    eaQHMNoiseSynthesis(noise, tau, L_out, seed=0, *, device_index=0) -> float64[L_out]
    noise_time_map(hop, L_out, rho) / noise_time_map_contour(hop, tm, step) -> float64[Nq]
    eaQHMNoiseWarp(noise, formant_scale=1.0, *, formant_warp=None, device_index=0) -> dict(sigma, refl, hop, order, fs, length)
    noise_formant_contour(noise, DetComponents, formant_scale) -> float64[Nf]
    noise_envelope(noise, fs, freqs, formant_scale=1.0, *, device_index=0) -> float64[Nf, len(freqs)]
    model_phase(DetComponents, fs, f0=None) -> float64[No_ti]
    eaQHMNoiseModulation(s, s_recon, noise, DetComponents, harmonics=2, f0=None, *, device_index=0) -> noise + mod
    noise_fundamental(DetComponents, fs, tau, time_map=None, time_scale=1.0, pitch_scale=1.0, f0=None) -> (theta, nu)

`DetComponents` is either form eaQHMAnalysisAndSynthesis returns: the list of Deterministic (det_format="structs") or
the dict of arrays (det_format="arrays"), edited or not.  At time_scale = pitch_scale = 1 the result is the analysis's
own s_recon; the definition for other settings is in DESIGN.md ("Resynthesis from the model", §9).  Either scale may
also be a contour, one value per analysis instant (§9.1).  A formant scale moves the spectral envelope on its own
(§9.2); a formant warp, a piecewise-linear frequency map (f_in, f_out) such as formant_warp_vtln's, moves it along a
curve instead of by one factor (§9.4, §10.3).  The residual s - s_recon is modelled apart, as an LPC envelope and a gain per 5 ms frame, and resynthesised as
filtered white noise under the same time map (§10); its envelope follows a formant scale on request (§10.1).  phase="shape" keeps the phases of the harmonics relative to the
fundamental, the waveform shape of a pitch period, at every scale (§11).  The work runs in libeaqhm_hip.so (eaqhm_spline_solve,
eaqhm_modify_prep, eaqhm_modify_synth, eaqhm_model_envelope, eaqhm_noise_analyse, eaqhm_noise_synth, eaqhm_noise_warp,
eaqhm_noise_envelope, eaqhm_noise_modulation, eaqhm_model_cepstrum, eaqhm_modify_amp_cepstrum, eaqhm_cepstrum_envelope,
eaqhm_cepstrum_cost, eaqhm_dtw, eaqhm_model_build, eaqhm_cepstrum_phase);
there is no CPU path.  A model can also be built from parameters alone, f0 and cepstral rows, with the minimum-phase response of
the envelope as the phases (§9.7): model_parameters reduces a model to such arrays, model_from_parameters is the way back.  The noise of voiced frames is modulated pitch-synchronously on request
(§10.2): eaQHMNoiseModulation adds the Fourier coefficients of the residual's power over the fundamental's phase to the
noise model, and the synthesis plays that envelope at the output's fundamental.
"""
from functools import partial
from itertools import chain, compress, repeat
from operator import itemgetter

import numpy as np

SCALE_RANGE = (0.25, 4.0)
NOISE_MAX_HOP = 1024     # the analysis kernel keeps one 4-hop frame per wave in LDS
NOISE_MAX_ORDER = 63     # lane l of a wave owns lag l
NOISE_MOD_MAX = 8        # harmonics of the pitch-synchronous envelope of the noise at most


def _cells(rows, mask=None):
    """Values of the SURVEY Q9 cells of every row that are not the int 0 of an inactive slot (shape-(1,) arrays), in
    row-major order, and the mask of those cells over all cells.  The cells are read by NumPy and itertools, not by a
    loop over them; `mask` (from the amplitudes) saves the type scan for the other two fields.  Cells edited by hand
    into plain numbers take a slower per-cell path."""
    if mask is None:
        flat = chain.from_iterable(r for r in rows if r is not None)
        mask = ~np.fromiter(map(isinstance, flat, repeat(int)), dtype=bool)
    n = int(np.count_nonzero(mask))
    try:
        v = np.fromiter(map(itemgetter(0), compress(chain.from_iterable(r for r in rows if r is not None), mask)),
                        dtype=np.float64, count=n)
    except (TypeError, IndexError, ValueError):
        v = np.array([np.asarray(c, dtype=np.float64).reshape(-1)[0] if np.size(c) == 1 else np.nan
                      for c in compress(chain.from_iterable(r for r in rows if r is not None), mask)])
        if np.isnan(v).any() or len(v) != n:
            raise ValueError("every cell of a Deterministic row must be a single number (a shape-(1,) array)") from None
    return v, mask


def unpack_model(DetComponents):
    """The inverse of functions.pack_results / pack_arrays: the model as records in the layout of include/eaqhm_hip.h
    (|a| (Kmax), f (Kmax), phase (Kmax), a0 per instant).

    A slot is active at an instant iff its amplitude is nonzero and its frequency is > 0; every other cell is zero.
    Cells with a nonzero amplitude and a frequency <= 0 are the reference's seeded slot-0 entries that reach the model
    when the loop stops in an adaptation that seeded empty rows (functions.py:210 through the aliasing at :383): the
    synthesis that produced s_recon never used them.  They come back inactive and are counted in `quirk_cells`.

    Returns dict(records=(No_ti, 3*Kmax+1) float64, step=int, Kmax=int, ti=int64[No_ti], quirk_cells=int)."""
    if isinstance(DetComponents, dict):
        d = DetComponents
        ti = np.asarray(d["ti"], dtype=np.int64).reshape(-1)
        am = np.array(d["amplitudes"], dtype=np.float64, ndmin=2)
        fm = np.array(d["frange"], dtype=np.float64, ndmin=2)
        pk = np.array(d["pk"], dtype=np.float64, ndmin=2)
        a0 = np.array(d["a0"], dtype=np.float64).reshape(-1)
        if not (am.shape == fm.shape == pk.shape) or am.shape[0] != len(ti) or len(a0) != len(ti):
            raise ValueError("det_format='arrays' model: amplitudes / frange / pk must be (No_ti, Kmax), a0 (No_ti,)")
        if "isVoiced" in d:
            v = np.asarray(d["isVoiced"], dtype=bool)
            am[~v] = 0.0
            a0 = np.where(v, a0, 0.0)
        n, K = am.shape
    else:
        det = list(DetComponents)
        n = len(det)
        ti = np.fromiter((int(x.ti) for x in det), dtype=np.int64, count=n)
        voiced = np.fromiter((bool(x.isVoiced) for x in det), dtype=bool, count=n)
        fields = []
        for name in ("amplitudes", "frange", "pk"):
            fields.append([getattr(x, name, None) if v else None for x, v in zip(det, voiced)])
        lens = np.array([0 if r is None else len(r) for r in fields[0]], dtype=np.int64)
        for rows in fields[1:]:
            if not np.array_equal(lens, [0 if r is None else len(r) for r in rows]):
                raise ValueError("amplitudes, frange and pk of an instant must have the same length")
        K = int(lens.max()) if n else 0
        a0 = np.array([float(x.a0) if v else 0.0 for x, v in zip(det, voiced)], dtype=np.float64)
        r_of = np.repeat(np.arange(n), lens)
        k_of = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
        am = np.zeros((n, K))
        fm = np.zeros((n, K))
        pk = np.zeros((n, K))
        mask = None
        flat_idx = r_of * K + k_of
        for out, rows in zip((am, fm, pk), fields):
            vals, mask = _cells(rows, mask)
            out.reshape(-1)[flat_idx[mask]] = vals
    if n < 2:
        raise ValueError("the model needs at least two analysis instants")
    step = int(ti[1] - ti[0])
    if step <= 0 or np.any(np.diff(ti) != step):
        raise ValueError("the model's instants ti must be uniformly spaced")
    if ti[0] != 0:
        raise ValueError("the model's first instant must be sample 0 (ti[0] == 0), as the analysis returns it")
    nonzero = am != 0
    active = nonzero & (fm > 0)
    quirk = int(np.count_nonzero(nonzero & ~active))
    rec = np.zeros((n, 3 * K + 1))
    rec[:, :K] = np.where(active, am, 0.0)
    rec[:, K:2 * K] = np.where(active, fm, 0.0)
    rec[:, 2 * K:3 * K] = np.where(active, pk, 0.0)
    rec[:, 3 * K] = a0
    return dict(records=rec, step=step, Kmax=int(K), ti=ti, quirk_cells=quirk)


def _scale(x, name):
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number" % name) from None
    if not np.isfinite(v) or not (SCALE_RANGE[0] <= v <= SCALE_RANGE[1]):
        raise ValueError("%s must be finite and in [%g, %g], got %r" % (name, SCALE_RANGE[0], SCALE_RANGE[1], x))
    return v


def _sample_rate(fs):
    try:
        fs = float(fs)
    except (TypeError, ValueError):
        raise ValueError("fs must be a number") from None
    if not np.isfinite(fs) or fs <= 0:
        raise ValueError("fs must be finite and > 0")
    return fs


def _is_contour(x):
    """True for an array-like scale (a contour); numbers and strings are scalars."""
    return not isinstance(x, (str, bytes)) and np.ndim(x) > 0


def _numeric_1d(x, name):
    a = np.asarray(x)
    if a.dtype.kind not in "iuf":
        raise ValueError("%s must hold numbers" % name)
    if a.ndim != 1:
        raise ValueError("%s must be 1-D, got shape %s" % (name, a.shape))
    return a.astype(np.float64)


def _in_range(v, name):
    if not np.all(np.isfinite(v)) or np.any(v < SCALE_RANGE[0]) or np.any(v > SCALE_RANGE[1]):
        raise ValueError("%s must be finite and in [%g, %g]" % (name, SCALE_RANGE[0], SCALE_RANGE[1]))
    return v


def _contour(x, name, n):
    """A scale as float64[n]: a number broadcast, or a 1-D array of n values."""
    if not _is_contour(x):
        return np.full(n, _scale(x, name))
    v = _numeric_1d(x, name)
    if len(v) != n:
        raise ValueError("%s must have one value per analysis instant (%d), got %d" % (name, n, len(v)))
    return _in_range(v, name)


def check_curve(times_s, values, name="curve"):
    """Validates a breakpoint curve (seconds, scale): returns (times, values) as float64 arrays.  The times must be
    finite and strictly increasing, the values finite and in SCALE_RANGE."""
    t = _numeric_1d(times_s, name + " times")
    v = _numeric_1d(values, name + " values")
    if len(t) == 0 or len(t) != len(v):
        raise ValueError("%s: times and values must be non-empty and of the same length" % name)
    if not np.all(np.isfinite(t)) or np.any(np.diff(t) <= 0):
        raise ValueError("%s: times must be finite and strictly increasing" % name)
    return t, _in_range(v, name + " values")


def _model_instants(DetComponents):
    if isinstance(DetComponents, dict):
        return np.asarray(DetComponents["ti"], dtype=np.float64).reshape(-1)
    return np.array([float(x.ti) for x in DetComponents], dtype=np.float64)


def scale_contour(DetComponents, fs, times_s, values):
    """The per-instant contour of a breakpoint curve, for eaQHMSynthesis's time_scale or pitch_scale: the curve
    (times_s in seconds, values in SCALE_RANGE) interpolated linearly at every analysis instant ti / fs of the model,
    held flat before the first and after the last breakpoint.  Returns float64[No_ti]."""
    t, v = check_curve(times_s, values)
    return np.interp(_model_instants(DetComponents) / _sample_rate(fs), t, v)


def contour_time_map(rho, beta, step, length):
    """The time map of DESIGN.md §9.1 for contours rho, beta (float64[n]) on knots c_i = i * step: per interval j
    r_j = (rho_j + rho_{j+1}) / 2 and g_j = r_j (beta_j + beta_{j+1}) / 2; the output knots C_0 = 0,
    C_{j+1} = C_j + r_j step (a float64 cumulative sum, the kernel's input); L_out = rint(C_{n-1} + rho_{n-1}
    (length - c_{n-1})).  Returns dict(rate=float64[n] (r_j, then rho_{n-1}), gain=float64[n-1], C=float64[n], L_out,
    rate_min)."""
    rho = np.asarray(rho, dtype=np.float64)
    beta = np.asarray(beta, dtype=np.float64)
    n = len(rho)
    r = (rho[:-1] + rho[1:]) / 2
    g = r * ((beta[:-1] + beta[1:]) / 2)
    C = np.concatenate(([0.0], np.cumsum(r * float(step))))
    L_out = int(np.rint(C[-1] + rho[-1] * (length - (n - 1) * step)))
    rate = np.append(r, rho[-1])
    return dict(rate=rate, gain=g, C=C, L_out=L_out, rate_min=float(rate.min()))


def check_arguments(model, fs, length, time_scale, pitch_scale):
    """Validates everything eaQHMSynthesis gets (no device work): returns (rho, beta, fs, length)."""
    rho = _scale(time_scale, "time_scale")
    beta = _scale(pitch_scale, "pitch_scale")
    fs = _sample_rate(fs)
    if isinstance(length, bool) or not float(length).is_integer():
        raise ValueError("length must be an integer number of samples")
    length = int(length)
    if length < int(model["ti"][-1]) + 1:
        raise ValueError("length (%d) must be >= the last instant + 1 (%d)" % (length, int(model["ti"][-1]) + 1))
    _check_records(model)
    return rho, beta, fs, length


def _check_records(model):
    rec = model["records"]
    if len(rec) < 4:
        raise ValueError("the model needs at least 4 analysis instants (the cubic interpolation of the tracks)")
    if not np.all(np.isfinite(rec)):
        raise ValueError("the model holds non-finite values")
    if np.any(rec[:, :model["Kmax"]] < 0):
        raise ValueError("amplitudes must be >= 0 (the model holds |a_k|)")


def check_contour_arguments(model, fs, length, time_scale, pitch_scale):
    """check_arguments for contours (no device work): either scale may be a number (broadcast) or a 1-D array of one
    value per analysis instant.  Returns (rho, beta, fs, length) with rho, beta float64[No_ti]."""
    n = len(model["ti"])
    rho = _contour(time_scale, "time_scale", n)
    beta = _contour(pitch_scale, "pitch_scale", n)
    _, _, fs, length = check_arguments(model, fs, length, 1.0, 1.0)
    return rho, beta, fs, length


def check_formant_scale(model, formant_scale, preserve_envelope):
    """Validates a formant scale (no device work): returns alpha as a float, or as float64[No_ti] for a contour.
    formant_scale != 1 needs the envelope it scales (preserve_envelope=True)."""
    if _is_contour(formant_scale):
        alpha = _contour(formant_scale, "formant_scale", len(model["ti"]))
        scaled = bool(np.any(alpha != 1.0))
    else:
        alpha = _scale(formant_scale, "formant_scale")
        scaled = alpha != 1.0
    if scaled and not preserve_envelope:
        raise ValueError("formant_scale != 1 needs preserve_envelope=True: there is no envelope to scale")
    return alpha


FORMANT_WARP_MAX = 16    # breakpoints of a formant warp at most: the kernels keep a row in 16 doubles of LDS per wave


def _warp_rows(formant_warp, rows, per):
    """A formant warp (f_in, f_out) as (float64[B], float64[rows, B]), validated: f_in is [B], f_out [B] or [rows, B]
    (one row per `per`), 1 <= B <= 16; all values finite and > 0; f_in and every row of f_out strictly increasing; every
    segment slope, the one from the origin included, in SCALE_RANGE."""
    try:
        f_in, f_out = formant_warp
    except (TypeError, ValueError):
        raise ValueError("formant_warp must be the pair (f_in, f_out) of breakpoint frequencies in Hz") from None
    x, y = np.asarray(f_in), np.asarray(f_out)
    if x.dtype.kind not in "iuf" or y.dtype.kind not in "iuf":
        raise ValueError("formant_warp must hold numbers")
    if x.ndim != 1:
        raise ValueError("formant_warp f_in must be 1-D, got shape %s" % (x.shape,))
    B = len(x)
    if not 1 <= B <= FORMANT_WARP_MAX:
        raise ValueError("formant_warp must have 1 to %d breakpoints, got %d" % (FORMANT_WARP_MAX, B))
    if y.shape != (B,) and y.shape != (rows, B):
        raise ValueError("formant_warp f_out must have shape (%d,) or one row per %s (%d, %d), got %s"
                         % (B, per, rows, B, y.shape))
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(np.broadcast_to(y, (rows, B)), dtype=np.float64)
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))) or np.any(x <= 0) or np.any(y <= 0):
        raise ValueError("formant_warp frequencies must be finite and > 0 (the map starts at (0, 0) by itself)")
    if np.any(np.diff(x) <= 0) or np.any(np.diff(y, axis=1) <= 0):
        raise ValueError("formant_warp f_in and every row of f_out must be strictly increasing")
    slope = np.diff(y, axis=1, prepend=0.0) / np.diff(x, prepend=0.0)
    if np.any(slope < SCALE_RANGE[0]) or np.any(slope > SCALE_RANGE[1]):
        raise ValueError("formant_warp: every segment slope (the one from the origin included) must be in [%g, %g]"
                         % SCALE_RANGE)
    return x, y


def _warp_excludes_scale(formant_scale):
    if _is_contour(formant_scale) or _scale(formant_scale, "formant_scale") != 1.0:
        raise ValueError("formant_warp and formant_scale exclude each other: B = 1 with (x, alpha x) is the scale alpha")


def check_formant_warp(model, fs, formant_warp, formant_scale=1.0, preserve_envelope=True):
    """Validates a formant warp (no device work): `formant_warp` = (f_in, f_out) in Hz, f_in [B] model
    frequencies, f_out [B] or [No_ti, B] (one row per analysis instant) output frequencies, 1 <= B <= 16, all finite and
    > 0, each strictly increasing, every segment slope (from the origin included) in [0.25, 4].  It excludes a
    formant_scale that is a contour or != 1 and needs preserve_envelope=True.  Returns (f_in float64[B],
    f_out float64[No_ti, B])."""
    _sample_rate(fs)
    _warp_excludes_scale(formant_scale)
    if not preserve_envelope:
        raise ValueError("formant_warp needs preserve_envelope=True: there is no envelope to warp")
    return _warp_rows(formant_warp, len(model["ti"]), "analysis instant")


def formant_warp_vtln(fs, alpha, knee=0.875):
    """The piecewise-linear map of vocal-tract length normalisation as a formant warp (host only): slope `alpha` from
    the origin up to the knee, then straight to (fs/2, fs/2), so the whole band of the model fills the whole band of the
    output.  The breakpoints are (f_k, alpha f_k) with f_k = knee (fs/2) min(1, 1/alpha), and (fs/2, fs/2).  Raises
    ValueError when `knee` is not in (0, 1) or either slope leaves [0.25, 4].  Returns (f_in, f_out), float64[2] each:
    eaQHMSynthesis's, model_envelope's, eaQHMNoiseWarp's and noise_envelope's `formant_warp`."""
    fs = _sample_rate(fs)
    alpha = _scale(alpha, "alpha")
    try:
        knee = float(knee)
    except (TypeError, ValueError):
        raise ValueError("knee must be a number") from None
    if not 0.0 < knee < 1.0:
        raise ValueError("knee must lie in (0, 1), got %r" % (knee,))
    nyq = fs / 2
    fk = knee * nyq * min(1.0, 1.0 / alpha)
    f_in, f_out = np.array([fk, nyq]), np.array([alpha * fk, nyq])
    upper = (f_out[1] - f_out[0]) / (f_in[1] - f_in[0])
    if not SCALE_RANGE[0] <= upper <= SCALE_RANGE[1]:
        raise ValueError("alpha %g with knee %g gives the slope %g above the knee, outside [%g, %g]"
                         % ((alpha, knee, upper) + SCALE_RANGE))
    return f_in, f_out


PHASE_MODES = ("independent", "shape")


def _records_f0(rec, K):
    """The fundamental track of DESIGN.md §11 from records: per instant the a^2-weighted mean of f_k / (k+1) over the
    active slots; an instant without one takes the nearest earlier instant's value that has one, else the nearest
    later one's; 0 everywhere for a model without any active slot."""
    am, fm = rec[:, :K], rec[:, K:2 * K]
    w = np.where((am != 0) & (fm > 0), am * am, 0.0)
    # sums in slot order (cumsum is sequential): trailing empty slots, which det_format="arrays" keeps and "structs"
    # drops, add exact zeros and leave f0 as it is
    den = np.cumsum(w, axis=1)[:, -1] if K else np.zeros(len(rec))
    has = den > 0
    n = len(rec)
    if not has.any():
        return np.zeros(n)
    num = np.cumsum(w * (fm / np.arange(1, K + 1)), axis=1)[:, -1]
    f0 = np.where(has, num / np.where(has, den, 1.0), 0.0)
    idx = np.where(has, np.arange(n), -1)
    src = np.maximum.accumulate(idx)                 # the nearest earlier instant with an active slot
    src[src < 0] = int(np.flatnonzero(has)[0])       # none earlier: the nearest later one
    return f0[src]


def model_f0(DetComponents, fs):
    """The fundamental frequency the model itself holds, in Hz per analysis instant: the a^2-weighted
    mean of f_k / (k+1) over the instant's active partials (slot k holds harmonic k+1), held over instants without any.
    It is what eaQHMSynthesis(..., phase="shape") advances, and what drives a pitch contour to a target:
    pitch_scale = target_hz / model_f0(det, fs).  Returns float64[No_ti]."""
    _sample_rate(fs)
    model = unpack_model(DetComponents)
    return _records_f0(model["records"], model["Kmax"])


def check_phase_arguments(model, phase, f0):
    """Validates the phase mode and the fundamental track (no device work): returns (shape: bool, f0: float64[No_ti]
    or None).  f0 is only allowed with phase="shape"; it must be finite and > 0 at every instant."""
    if phase not in PHASE_MODES:
        raise ValueError("phase must be one of %s, got %r" % (", ".join(map(repr, PHASE_MODES)), phase))
    shape = phase == "shape"
    if f0 is None:
        return shape, (_records_f0(model["records"], model["Kmax"]) if shape else None)
    if not shape:
        raise ValueError("f0 is the fundamental track of phase='shape'; it has no meaning with phase=%r" % phase)
    v = _numeric_1d(f0, "f0")
    if len(v) != len(model["ti"]):
        raise ValueError("f0 must have one value per analysis instant (%d), got %d" % (len(model["ti"]), len(v)))
    if not np.all(np.isfinite(v)) or np.any(v <= 0):
        raise ValueError("f0 must be finite and > 0 (Hz)")
    return shape, v


def fundamental_advance(f0, gain, step, fs):
    """S of DESIGN.md §11: the phase advance of the fundamental in cycles at every instant, S_0 = 0,
    S_{j+1} = frac(S_j + (g_j - 1) (step / fs) (f0_j + f0_{j+1}) / 2), in float64 in this order.  `gain` is g_j per
    interval (float64[n-1]).  frac keeps (k+1) S small whatever the length of the file.  Returns float64[n] in [0, 1)."""
    f0 = np.asarray(f0, dtype=np.float64)
    inc = (np.asarray(gain, dtype=np.float64) - 1.0) * (float(step) / float(fs)) * (f0[:-1] + f0[1:]) / 2
    S = np.zeros(len(f0))
    acc = 0.0
    for j, d in enumerate(inc.tolist()):
        acc += d
        acc -= np.floor(acc)
        S[j + 1] = acc
    return S


def _device(device_index):
    """(torch, the library context of the device bound to torch's current stream, its torch.device)."""
    import torch
    from .functions import _ctx
    c = _ctx(device_index)
    return torch, c, c.device


def _device_records(model, dev):
    """The model's records on the device: (tensor, No_ti, Kmax).  A model without any slot keeps one empty slot, so that
    the kernels still run (the a0 spline of the synthesis, the -inf rows of the envelope)."""
    import torch
    rec_h = model["records"]
    n, K = rec_h.shape[0], model["Kmax"]
    if K == 0:
        rec_h = np.concatenate((np.zeros((n, 3)), rec_h), axis=1)
        K = 1
    return torch.as_tensor(np.ascontiguousarray(rec_h), device=dev), n, K


def eaQHMSynthesis(DetComponents, fs, length, time_scale=1.0, pitch_scale=1.0, preserve_envelope=True,
                   formant_scale=1.0, *, phase="independent", f0=None, noise=None, noise_seed=0, noise_formant=False,
                   noise_modulation=False, formant_warp=None, envelope=None, cep_warp=0.0, device_index=0,
                   _ranges=None):
    """Synthesises the model at `time_scale` (durations multiplied by it) and `pitch_scale` (every instantaneous
    frequency multiplied by it), both in [0.25, 4].  With `preserve_envelope` the amplitude of a scaled partial is read
    off the instant's log-amplitude envelope at its new frequency (the formants stay put); without it each partial keeps
    its own amplitude.  Partials pushed to or above fs/2 are muted.

    Each scale is either a number (the result has rint(time_scale * length) samples) or a contour: a 1-D
    array of one value per analysis instant of the model (len(det) for det_format="structs", len(det["ti"]) for
    "arrays"), e.g. from scale_contour().  If either is a contour the other is broadcast and the contour path runs
    (§9.1): interval j between two instants is stretched by the mean of their time scales and its frequencies are
    multiplied by the mean of their pitch scales; the length is contour_time_map(...)["L_out"].

    `formant_scale` (alpha, in [0.25, 4]; a number or a contour like the others) multiplies the frequencies of the
    spectral envelope: a formant at F in the model sits at alpha * F in the output, whatever the pitch does (§9.2).
    Each partial's amplitude is read off its instant's envelope at (pitch_scale * f) / alpha; phases, durations and
    the length do not change.  It needs preserve_envelope=True.  A formant contour runs the contour path; the number 1
    leaves the result exactly as it is without a formant scale.

    `phase` is "independent" (the default: the unwrapped phase of every partial is scaled on its own, §9) or "shape"
    (§11): the phase of harmonic k+1 relative to the fundamental, which fixes the waveform shape of a pitch period,
    stays the model's at every scale, and only the fundamental's phase advances at the new rate; stretched voiced speech
    keeps its pulse shape instead of turning reverberant.  The fundamental is model_f0(DetComponents, fs), or `f0` (Hz
    per analysis instant, finite and > 0; only with phase="shape").  At unit scales both modes give the same samples.

    `noise` (a model from eaQHMNoiseAnalysis of the same signal: its fs and length must be this call's) adds the
    stochastic component (§10): the LPC model of the residual resynthesised as filtered white noise, seeded by
    `noise_seed`, under this call's time map, so it is stretched with the sinusoids.  `pitch_scale` does not touch the
    noise, and neither does `formant_scale` by default.  The result is the sum of the synthesis without `noise` and
    eaQHMNoiseSynthesis at noise_time_map(...) (noise_time_map_contour for contours), bit for bit.

    `noise_formant=True` (it needs `noise` and preserve_envelope=True) lets the noise follow the formant scale (§10.1):
    the noise is synthesised from eaQHMNoiseWarp(noise, noise_formant_contour(noise, DetComponents, formant_scale)),
    the model whose all-pole envelope is moved up in frequency by alpha, so the result is bit for bit that of passing
    that warped model as `noise`.  The default leaves the noise's envelope where the analysis found it.

    `noise_modulation=True` (it needs `noise` with the `mod` of eaQHMNoiseModulation) modulates the noise
    pitch-synchronously (§10.2): the bursts of the analysed noise follow the fundamental this call plays, at every
    scale and in both phase modes.  The result is bit for bit the synthesis without noise plus eaQHMNoiseSynthesis(noise,
    tau, L_out, noise_seed, fundamental=noise_fundamental(DetComponents, fs, tau, ...)).  The default ignores `mod`.

    `formant_warp` = (f_in, f_out) generalises the formant scale from a number to a map (§9.4): a strictly increasing
    piecewise-linear map W through (0, 0) and the breakpoints (f_in[j], f_out[j]) in Hz, continued past the last one
    with its slope; a feature at F in the model sits at W(F) in the output, and each partial's amplitude is read off its
    instant's envelope at W^-1(pitch_scale * f).  f_in is [B], f_out [B] or [No_ti, B] (a map per analysis instant),
    1 <= B <= 16, every slope in [0.25, 4]; formant_warp_vtln builds the VTLN map.  It excludes a formant_scale != 1 and
    needs preserve_envelope=True; the length and the path (scalar or contour) are those of the time and pitch scales.
    With noise_formant=True the noise is synthesised from eaQHMNoiseWarp(noise, formant_warp=noise_formant_warp(noise,
    DetComponents, formant_warp)) (§10.3), bit for bit as if that model were passed as `noise`.  None leaves every
    result as it is.

    `envelope` = C, float64[No_ti, P + 1] with 1 <= P <= 63, supplies the spectral envelope as a discrete cepstrum per
    analysis instant (§9.5; model_cepstrum fits one, of this model or of another): every partial's amplitude is
    exp(C_i(q)) with q the frequency the model's own envelope would be read at (pitch_scale * f, divided by the formant
    scale or taken through W^-1), also at unit scales, since the envelope is the caller's and not the model's.  Entries
    are finite, except that a whole row may be (-inf, 0, .., 0): an instant without amplitude.  It needs
    preserve_envelope=True and goes with every scale, contour, formant_warp, phase mode and noise option; the noise
    options keep following the formant scale or warp and never read C.  None leaves every result as it is.

    `cep_warp` = a, |a| <= 0.9, says that the rows of `envelope` lie on the all-pass warped axis of §9.8
    (model_cepstrum(cep_warp=a) fits such rows): the read frequency is formed in Hz as above and then warped, so every
    scale and map keeps its meaning.  It needs `envelope`; 0, the default, is the linear axis and today's result.

    `_ranges` (tests): a list of (t_lo, t_hi) output ranges computed one after the other into the same buffer.
    Returns float64[L_out]."""
    model = unpack_model(DetComponents)
    contour = _is_contour(time_scale) or _is_contour(pitch_scale) or _is_contour(formant_scale)
    if contour:
        rho, beta, fs, length = check_contour_arguments(model, fs, length, time_scale, pitch_scale)
    else:
        rho, beta, fs, length = check_arguments(model, fs, length, time_scale, pitch_scale)
    alpha = check_formant_scale(model, formant_scale, preserve_envelope)
    wmap = None if formant_warp is None else check_formant_warp(model, fs, formant_warp, formant_scale,
                                                                preserve_envelope)
    shape, f0 = check_phase_arguments(model, phase, f0)
    ceps = None if envelope is None else check_envelope_cepstrum(model, envelope, preserve_envelope)
    axis = check_cepstrum_warp(cep_warp)
    if axis != 0.0 and ceps is None:
        raise ValueError("cep_warp says which axis the rows of envelope= lie on: it needs envelope=")
    # alpha reaches the prep for a formant contour or a number != 1; without the envelope alpha is 1 throughout
    formant = bool(preserve_envelope) and (_is_contour(formant_scale) or alpha != 1.0)
    if noise is not None:
        nz = check_noise_model(noise)
        seed = _seed(noise_seed)
        if nz["fs"] != fs or nz["length"] != length:
            raise ValueError("the noise model is of another signal: fs %g, length %d; this call: fs %g, length %d"
                             % (nz["fs"], nz["length"], fs, length))
    warp = check_noise_formant(noise_formant, noise, preserve_envelope)
    modulate = check_noise_modulation(noise_modulation, nz if noise is not None else None)
    torch, c, dev = _device(device_index)
    rec, n, K = _device_records(model, dev)
    D = model["step"]
    if contour:
        tm = contour_time_map(rho, beta, D, length)
        L_out = tm["L_out"]
    else:
        L_out = int(np.rint(rho * length))
    code = torch.empty(n * K, dtype=torch.uint8, device=dev)
    mom = torch.empty(n * (K + 1), dtype=torch.float64, device=dev)
    amp = torch.empty(n * K, dtype=torch.float64, device=dev)
    R = torch.empty(n * K, dtype=torch.float64, device=dev)
    ph0 = torch.empty(n * K, dtype=torch.float64, device=dev)
    out = torch.empty(L_out, dtype=torch.float64, device=dev)
    ranges = [(0, L_out)] if _ranges is None else [(int(a), int(b)) for a, b in _ranges]
    c.spline_solve(rec, n, K, D, code, mom)

    def dv(x):   # float64 on the device; a number becomes one value per instant
        return torch.as_tensor(np.full(n, x) if np.ndim(x) == 0 else np.ascontiguousarray(x), device=dev)

    gain_d = dv(tm["gain"]) if contour else None      # without it Delta stays unweighted: the scalar synthesis
    # phase="shape" leaves Delta unweighted on either path: the weight moves to the fundamental's advance S
    beta_d = dv(beta)
    if ceps is not None:   # as for the warp: the prep runs without the envelope and the cepstrum kernel writes amp
        c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, None if shape else gain_d, None, False, amp, R, ph0)
        _on_axis(c, "modify_amp_cepstrum", axis)(rec, n, K, fs, beta_d, dv(ceps), ceps.shape[1] - 1, amp,
                                                 alpha=dv(alpha) if formant else None,
                                                 warp=None if wmap is None else (dv(wmap[0]), dv(wmap[1]),
                                                                                 len(wmap[0])))
    elif wmap is None:
        c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, None if shape else gain_d, dv(alpha) if formant else None,
                      preserve_envelope, amp, R, ph0)
    else:   # R and ph0 do not depend on the envelope: the prep runs without it and the warp kernel writes amp
        c.modify_prep(rec, code, mom, n, K, D, fs, beta_d, None if shape else gain_d, None, False, amp, R, ph0)
        c.modify_amp_warp(rec, n, K, fs, beta_d, dv(wmap[0]), dv(wmap[1]), len(wmap[0]), amp)
    # the two optional groups of eaqhm_modify_synth; the contour map holds rho and beta, which are then not read
    curve_d = (dv(tm["C"]), dv(tm["rate"]), gain_d, tm["rate_min"]) if contour else None
    shape_d = None
    if shape:
        shape_d = (dv(f0), dv(fundamental_advance(f0, tm["gain"] if contour else np.full(n - 1, beta * rho), D, fs)))
    rho_s, beta_s = (0.0, 0.0) if contour else (rho, beta)
    for t_lo, t_hi in ranges:
        c.modify_synth(rec, code, mom, amp, R, ph0, n, K, D, fs, rho_s, beta_s, L_out, t_lo, t_hi, out, curve_d, shape_d)
    if noise is not None:
        H = nz["hop"]
        tau = noise_time_map_contour(H, tm, D) if contour else noise_time_map(H, L_out, rho)
        sigma_d, refl_d, tau_d = (torch.as_tensor(x, device=dev) for x in (nz["sigma"], nz["refl"], tau))
        if warp and wmap is not None:
            sigma_d, refl_d = _device_noise_warp_map(c, sigma_d, refl_d, nz["order"], *_warp_normalised(
                wmap[0], _frame_rows(nz, model["ti"], wmap[1]), fs))
        elif warp:
            sigma_d, refl_d = _device_noise_warp(c, sigma_d, refl_d, nz["order"],
                                                 _frame_alpha(nz, model["ti"], np.broadcast_to(alpha, (n,))))
        mod_d = None
        if modulate:
            f0m = f0 if f0 is not None else _records_f0(model["records"], model["Kmax"])
            path = (tm["gain"], tm["rate"], tm["rate"][-1] * beta[-1]) if contour else _scalar_path(n, rho, beta)
            theta, nu = _fundamental_at(model, fs, tau, f0m, *path)
            mod_d = _device_mod(torch, dev, nz, theta, nu)
        for t_lo, t_hi in ranges:
            c.noise_synth(sigma_d, refl_d, len(nz["sigma"]), H, nz["order"], tau_d, len(tau), seed, L_out, t_lo, t_hi, out,
                          accumulate=True, mod=mod_d)
    return out.cpu().numpy()


def _freq_grid(freqs):
    f = _numeric_1d(freqs, "freqs")
    if len(f) == 0 or len(f) > 2 ** 31 - 1 or not np.all(np.isfinite(f)) or np.any(f < 0):
        raise ValueError("freqs must be a non-empty 1-D array of finite frequencies >= 0 (Hz)")
    return f


def check_envelope_arguments(model, fs, freqs, formant_scale):
    """Validates everything model_envelope gets (no device work): returns (alpha float64[No_ti], freqs float64[F])."""
    _sample_rate(fs)
    f = _freq_grid(freqs)
    if len(model["records"]) < 4:
        raise ValueError("the model needs at least 4 analysis instants")
    _check_records(model)
    alpha = check_formant_scale(model, formant_scale, True)
    return np.array(np.broadcast_to(alpha, (len(model["ti"]),)), dtype=np.float64), f


def model_envelope(DetComponents, fs, freqs, formant_scale=1.0, formant_warp=None, *, device_index=0):
    """The log-amplitude envelope of every analysis instant on a frequency grid: out[i, t] = E_i(freqs[t] / alpha_i)
    (DESIGN.md §9.2), the natural log of the amplitude |a|, not muted at Nyquist.  E_i interpolates ln |a| linearly
    between the instant's active partials ordered by frequency and is flat outside them; rows of instants without
    active partials are -inf.  With formant_scale = alpha (a number or one value per instant, in [0.25, 4]) it is the
    envelope eaQHMSynthesis reads the amplitudes from at that formant scale.  `freqs` (Hz) is 1-D, finite and >= 0.

    With `formant_warp` = (f_in, f_out) (eaQHMSynthesis's; §9.4) it is out[i, t] = E_i(W_i^-1(freqs[t])) instead, the
    envelope the synthesis reads under that map; it excludes a formant_scale != 1.

    The result takes No_ti * len(freqs) * 8 bytes, once on the device and once on the host (61 MB for a 60 s model at
    16 kHz, step 15, 64 000 instants, on a 120-point grid).  Returns float64[No_ti, len(freqs)]."""
    model = unpack_model(DetComponents)
    alpha, f = check_envelope_arguments(model, fs, freqs, formant_scale)
    wmap = None if formant_warp is None else check_formant_warp(model, fs, formant_warp, formant_scale, True)
    torch, c, dev = _device(device_index)
    rec, n, K = _device_records(model, dev)
    f_d = torch.as_tensor(np.ascontiguousarray(f), device=dev)
    out = torch.empty((n, len(f)), dtype=torch.float64, device=dev)
    if wmap is None:
        alpha_d = torch.as_tensor(np.ascontiguousarray(alpha), device=dev)
        c.model_envelope(rec, n, K, alpha_d, f_d, len(f), out)
    else:
        x_d, y_d = (torch.as_tensor(v, device=dev) for v in wmap)
        c.model_envelope_warp(rec, n, K, x_d, y_d, len(wmap[0]), f_d, len(f), out)
    return out.cpu().numpy()


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


# ---- time alignment of two models
def band_centres(nA, nB):
    """c_i = (2 i (nB-1) + (nA-1)) // (2 (nA-1)), int64[nA]: the row of B on the scaled diagonal at row i of A (0 when
    nA = 1)."""
    i = np.arange(nA, dtype=np.int64)
    if nA == 1:
        return np.zeros(1, dtype=np.int64)
    return (2 * i * np.int64(nB - 1) + np.int64(nA - 1)) // np.int64(2 * (nA - 1))


def band_min_radius(nA, nB):
    """The smallest half-width that admits a path: nB - 1 when nA = 1, else ceil((nB - 1) / (nA - 1))."""
    return nB - 1 if nA == 1 else -((1 - nB) // (nA - 1))


def _band_radius(band, nA, nB):
    """band=None is the full table, r = max(nA, nB) - 1; an integer is r itself (never more than the full table)."""
    full = max(nA, nB) - 1
    if band is None:
        return full
    r = _integer(band, "band")
    if r < band_min_radius(nA, nB):
        raise ValueError("band=%d admits no path between %d and %d rows: it needs band >= %d"
                         % (r, nA, nB, band_min_radius(nA, nB)))
    return min(r, full)


def dense_to_band(cost, r):
    """A dense float64[nA, nB] table in band layout float64[nA, 2 r + 1]: cell (i, j) at [i, j - c_i + r], +inf where
    the band leaves the table."""
    cost = np.asarray(cost, dtype=np.float64)
    nA, nB = cost.shape
    j = band_centres(nA, nB)[:, None] - r + np.arange(2 * r + 1, dtype=np.int64)[None, :]
    inside = (j >= 0) & (j < nB)
    out = np.full(j.shape, np.inf)
    out[inside] = cost[np.nonzero(inside)[0], j[inside]]
    return out


def _run_dtw(torch, c, band_d, nA, nB, r):
    """eaqhm_dtw on a device band: (path int64[L, 2], total)."""
    dev = c.device
    ptr = torch.empty(band_d.shape, dtype=torch.uint8, device=dev)
    path = torch.empty((nA + nB - 1, 2), dtype=torch.int32, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    c.dtw(band_d, nA, nB, r, ptr, path, n, total)
    L = int(n.item())
    if L < 1:
        raise RuntimeError("the alignment's back-pointers do not lead back to the start")
    return path[:L].cpu().numpy().astype(np.int64), float(total.item())


def _fits_device(torch, dev, nA, r):
    """The working set of an alignment, the band of costs and its back-pointers, 9 bytes per cell."""
    need = 9 * nA * (2 * r + 1)
    free = torch.cuda.mem_get_info(dev)[0]
    if need > free:
        raise ValueError("the alignment needs %d bytes for %d x %d band cells and the device has %d free: pass a "
                         "narrower band=" % (need, nA, 2 * r + 1, free))


def _cost_weight(x, name):
    try:
        x = float(x)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number" % name) from None
    if not (np.isfinite(x) and x >= 0):
        raise ValueError("%s must be finite and >= 0, got %r" % (name, x))
    return x


def check_model_align_arguments(CA, CB, band=None, c0_weight=0.0, empty_cost=4.0):
    """Validates everything model_align gets (no device work): returns (CA, CB, r, c0_weight, empty_cost)."""
    CA, CB = _cepstrum_rows(CA, "CA"), _cepstrum_rows(CB, "CB")
    if CA.shape[1] != CB.shape[1]:
        raise ValueError("CA and CB must have the same order, got %d and %d" % (CA.shape[1] - 1, CB.shape[1] - 1))
    return (CA, CB, _band_radius(band, len(CA), len(CB)), _cost_weight(c0_weight, "c0_weight"),
            _cost_weight(empty_cost, "empty_cost"))


def model_align(CA, CB, band=None, c0_weight=0.0, empty_cost=4.0, *, device_index=0):
    """Aligns two cepstra in time by dynamic time warping.  `CA` float64[nA, P + 1] and `CB`
    float64[nB, P + 1] are model_cepstrum's rows (or any such rows) of the same order.  The cost of pairing row i of A
    with row j of B is d = c0_weight dC_0^2 + 2 sum_p dC_p^2, dC = CA[i] - CB[j]: at c0_weight = 1 the mean over
    frequency of the squared difference of the two log envelopes; the default 0 ignores the level.  Two empty rows
    (-inf, 0, .., 0) cost 0, an empty row against any other `empty_cost`.  `band` is the half-width, in rows of B,
    around the straight line from (0, 0) to (nA - 1, nB - 1) that the path may use; None is the whole table.  Returns
    (path, cost): int64[L, 2], the pairs (i, j) from (0, 0) to (nA - 1, nB - 1) in steps of (1, 1), (1, 0), (0, 1),
    with the smallest sum of d, and that sum.  On equal sums the diagonal step is preferred, then (1, 0).  Raises
    ValueError when `band` admits no path or the band does not fit the device's free memory."""
    CA, CB, r, c0_weight, empty_cost = check_model_align_arguments(CA, CB, band, c0_weight, empty_cost)
    nA, nB, P = len(CA), len(CB), CA.shape[1] - 1
    torch, c, dev = _device(device_index)
    _fits_device(torch, dev, nA, r)
    band_d = torch.empty((nA, 2 * r + 1), dtype=torch.float64, device=dev)
    c.cepstrum_cost(torch.as_tensor(CA, device=dev), nA, torch.as_tensor(CB, device=dev), nB, P, c0_weight, empty_cost,
                    r, band_d)
    return _run_dtw(torch, c, band_d, nA, nB, r)


def check_dtw_arguments(cost, band=None):
    """Validates dtw's arguments (no device work): returns (cost float64[nA, nB], r)."""
    D = np.asarray(cost)
    if D.dtype.kind not in "iuf" or D.ndim != 2 or D.shape[0] < 1 or D.shape[1] < 1:
        raise ValueError("cost must be a 2-D array of numbers, one row per row of A and one column per row of B")
    D = np.ascontiguousarray(D, dtype=np.float64)
    if not np.all(np.isfinite(D)) or np.any(D < 0):
        raise ValueError("cost must be finite and >= 0")
    return D, _band_radius(band, *D.shape)


def dtw(cost, band=None, *, device_index=0):
    """Dynamic time warping over the caller's own costs: `cost` float64[nA, nB], finite and >= 0 (for instance
    model_align's cost plus an f0 or voicing term).  `band`, the path and the tie rule are model_align's.  Returns
    (path int64[L, 2], total)."""
    D, r = check_dtw_arguments(cost, band)
    nA, nB = D.shape
    torch, c, dev = _device(device_index)
    _fits_device(torch, dev, nA, r)
    return _run_dtw(torch, c, torch.as_tensor(dense_to_band(D, r), device=dev), nA, nB, r)


def _path(path, nA):
    p = np.asarray(path)
    nA = _integer(nA, "nA")
    if p.dtype.kind not in "iu" or p.ndim != 2 or p.shape[1] != 2 or len(p) < 1:
        raise ValueError("path must be an integer array [L, 2] of pairs (i, j)")
    if nA < 1 or p[:, 0].min() < 0 or p[:, 0].max() >= nA or p[:, 1].min() < 0:
        raise ValueError("path must pair instants 0..%d of A with instants >= 0 of B" % (nA - 1))
    count = np.bincount(p[:, 0], minlength=nA)
    if np.any(count == 0):
        raise ValueError("path leaves instant %d of A unmatched" % int(np.flatnonzero(count == 0)[0]))
    return p, count


def alignment_index(path, nA):
    """For each instant of A the mean of the B indices the path pairs with it: float64[nA], fractional where an
    instant of A is held over several of B.  warp_rows reads B's rows there."""
    p, count = _path(path, nA)
    return np.bincount(p[:, 0], weights=p[:, 1].astype(np.float64), minlength=len(count)) / count


def warp_rows(X, idx):
    """The rows of `X` (1-D: its entries) read at the fractional row indices `idx` by linear interpolation between the
    two neighbouring rows; indices are held at the ends; an integer index returns the row bit for bit.  A 2-D `X` may
    hold empty cepstral rows (-inf, 0, .., 0): the nearer neighbour decides (the lower one at a fraction of exactly
    0.5): the result is the empty row when it is empty, and a copy of it when only the farther one is.  Returns
    float64[len(idx)] or float64[len(idx), X.shape[1]], e.g. warp_rows(CB, alignment_index(path, len(CA))): B's
    envelope at A's instants."""
    X = np.asarray(X)
    if X.dtype.kind not in "iuf" or X.ndim not in (1, 2) or len(X) < 1:
        raise ValueError("X must be a 1-D or 2-D array of numbers with at least one row")
    X = X.astype(np.float64)
    t = _numeric_1d(idx, "idx")
    if not np.all(np.isfinite(t)):
        raise ValueError("idx must be finite")
    t = np.clip(t, 0.0, len(X) - 1.0)
    lo = np.floor(t).astype(np.int64)
    hi = np.minimum(lo + 1, len(X) - 1)
    u = t - lo
    near = np.where(u > 0.5, hi, lo)
    w = u if X.ndim == 1 else u[:, None]
    with np.errstate(invalid="ignore"):
        out = (1.0 - w) * X[lo] + w * X[hi]
    whole = u == 0.0
    out[whole] = X[lo[whole]]
    if X.ndim == 2:
        empty = np.isneginf(X[:, 0])
        copy = ~whole & (empty[lo] | empty[hi])
        out[copy] = X[near[copy]]
    return out


def alignment_time_scale(path, nA, step_ratio=1.0):
    """A time_scale contour that gives A the local tempo of B: clip(step_ratio * d alignment_index / d instant, 0.25,
    4), float64[nA] (numpy.gradient).  `step_ratio` is B's analysis step over A's.  The clip to eaQHMSynthesis's
    range makes the total length approximate: where B holds or skips more than a factor 4 the contour saturates."""
    try:
        step_ratio = float(step_ratio)
    except (TypeError, ValueError):
        raise ValueError("step_ratio must be a number") from None
    if not (np.isfinite(step_ratio) and step_ratio > 0):
        raise ValueError("step_ratio must be finite and > 0")
    idx = alignment_index(path, nA)
    if len(idx) < 2:
        raise ValueError("a time-scale contour needs at least two instants of A")
    return np.clip(step_ratio * np.gradient(idx), *SCALE_RANGE)


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


# ---- the stochastic component
def _integer(x, name):
    if isinstance(x, (bool, np.bool_)):
        raise ValueError("%s must be an integer" % name)
    try:
        ok = float(x).is_integer()
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("%s must be an integer, got %r" % (name, x))
    return int(x)


def _seed(seed):
    seed = _integer(seed, "seed")
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2**64)")
    return seed


def _noise_shape(hop, order):
    if not 1 <= hop <= NOISE_MAX_HOP:
        raise ValueError("hop must be in [1, %d], got %d" % (NOISE_MAX_HOP, hop))
    if not 1 <= order <= NOISE_MAX_ORDER or order >= 4 * hop:
        raise ValueError("order must be in [1, %d] and < 4 * hop (%d), got %d" % (NOISE_MAX_ORDER, 4 * hop, order))


def _signal_pair(s, s_recon):
    a = _numeric_1d(s, "s")
    b = _numeric_1d(s_recon, "s_recon")
    if len(a) == 0 or len(a) != len(b):
        raise ValueError("s and s_recon must be non-empty and of the same length, got %d and %d" % (len(a), len(b)))
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        raise ValueError("s and s_recon must be finite")
    return a, b


def check_noise_analysis_arguments(s, s_recon, fs, order=None, hop=None):
    """Validates everything eaQHMNoiseAnalysis gets (no device work): returns (e, fs, hop, order) with the residual
    e = s - s_recon as float64.  hop defaults to round(0.005 fs), order to min(63, 2 + round(fs / 1000))."""
    fs = _sample_rate(fs)
    a, b = _signal_pair(s, s_recon)
    hop = int(round(0.005 * fs)) if hop is None else _integer(hop, "hop")
    order = min(NOISE_MAX_ORDER, 2 + int(round(fs / 1000.0))) if order is None else _integer(order, "order")
    _noise_shape(hop, order)
    return a - b, fs, hop, order


def check_noise_model(noise):
    """Validates a noise model (no device work): returns it with sigma float64[Nf] (finite, >= 0), refl
    float64[Nf, order] (|k| < 1) contiguous, hop, order and length ints, fs a float, Nf = (length - 1) // hop + 1.
    A model with the modulation of eaQHMNoiseModulation also returns mod float64[Nf, 2 M] (finite,
    contiguous) and mod_harmonics = M in [1, 8]; the two keys come together or not at all."""
    if not isinstance(noise, dict) or not all(k in noise for k in ("sigma", "refl", "hop", "order", "fs", "length")):
        raise ValueError("a noise model is the dict eaQHMNoiseAnalysis returns: sigma, refl, hop, order, fs, length")
    hop, order, length = (_integer(noise[k], k) for k in ("hop", "order", "length"))
    _noise_shape(hop, order)
    fs = _sample_rate(noise["fs"])
    sigma = _numeric_1d(noise["sigma"], "sigma")
    refl = np.asarray(noise["refl"])
    if refl.dtype.kind not in "iuf" or refl.ndim != 2:
        raise ValueError("refl must be a 2-D array of numbers")
    refl = np.ascontiguousarray(refl, dtype=np.float64)
    if length < 1 or len(sigma) != (length - 1) // hop + 1 or refl.shape != (len(sigma), order):
        raise ValueError("a noise model of %d samples at hop %d has %d frames: sigma must be (Nf,), refl (Nf, %d)"
                         % (length, hop, (max(length, 1) - 1) // hop + 1, order))
    if not np.all(np.isfinite(sigma)) or np.any(sigma < 0):
        raise ValueError("sigma must be finite and >= 0")
    if not np.all(np.abs(refl) < 1):     # also rejects NaN
        raise ValueError("reflection coefficients must lie inside (-1, 1)")
    out = dict(sigma=np.ascontiguousarray(sigma), refl=refl, hop=hop, order=order, fs=fs, length=length)
    if "mod" in noise or "mod_harmonics" in noise:
        if not ("mod" in noise and "mod_harmonics" in noise):
            raise ValueError("a modulated noise model holds both mod and mod_harmonics")
        M = _mod_harmonics(noise["mod_harmonics"], "mod_harmonics")
        mod = np.asarray(noise["mod"])
        if mod.dtype.kind not in "iuf" or mod.shape != (len(sigma), 2 * M):
            raise ValueError("mod must be a (Nf, 2 mod_harmonics) = (%d, %d) array of numbers" % (len(sigma), 2 * M))
        mod = np.ascontiguousarray(mod, dtype=np.float64)
        if not np.all(np.isfinite(mod)):
            raise ValueError("mod must be finite")
        out.update(mod=mod, mod_harmonics=M)
    return out


def check_noise_synthesis_arguments(noise, tau, L_out, seed=0):
    """Validates everything eaQHMNoiseSynthesis gets (no device work): returns (model, tau, L_out, seed); tau is
    float64[(L_out - 1) // hop + 1], finite and >= 0."""
    nz = check_noise_model(noise)
    L_out = _integer(L_out, "L_out")
    if L_out < 1:
        raise ValueError("L_out must be >= 1")
    tau = _numeric_1d(tau, "tau")
    Nq = (L_out - 1) // nz["hop"] + 1
    if len(tau) != Nq:
        raise ValueError("tau must have one value per output frame ((L_out - 1) // hop + 1 = %d), got %d"
                         % (Nq, len(tau)))
    if not np.all(np.isfinite(tau)) or np.any(tau < 0):
        raise ValueError("tau must be finite and >= 0")
    return nz, np.ascontiguousarray(tau), L_out, _seed(seed)


def noise_time_map(hop, L_out, rho):
    """tau of eaQHMNoiseSynthesis for a time scale rho: output frame centre q hop lies at (q hop) / rho of the analysed
    signal.  Returns float64[(L_out - 1) // hop + 1]."""
    return (np.arange((int(L_out) - 1) // int(hop) + 1, dtype=np.float64) * float(hop)) / float(rho)


def noise_time_map_contour(hop, tm, step):
    """tau of eaQHMNoiseSynthesis for a contour: the inverse of contour_time_map's map (`tm`) at the output frame
    centres x = q hop.  With j the last knot at or before x (C_j <= x), tau = j step + (x - C_j) / rate_j; past the
    last knot rate is rho_{n-1}, as contour_time_map stores it."""
    x = np.arange((int(tm["L_out"]) - 1) // int(hop) + 1, dtype=np.float64) * float(hop)
    C = np.asarray(tm["C"], dtype=np.float64)
    j = np.clip(np.searchsorted(C, x, side="right") - 1, 0, len(C) - 1)
    return j * float(step) + (x - C[j]) / np.asarray(tm["rate"], dtype=np.float64)[j]


def eaQHMNoiseAnalysis(s, s_recon, fs, order=None, hop=None, *, device_index=0):
    """The stochastic component of a signal: an all-pole (LPC) envelope and a gain for every frame of
    the residual e = s - s_recon.  `s` is the signal the analysis saw (read_signal(wav, fc)[1]), `s_recon` what
    eaQHMAnalysisAndSynthesis returned for it.  Frames are `hop` samples apart (default round(0.005 fs): 5 ms) and
    4 hop long (Hann); `order` (default min(63, 2 + round(fs / 1000))) is at most 63 and below 4 hop.

    Returns dict(sigma=float64[Nf] the standard deviation of the white excitation (0: a silent frame),
    refl=float64[Nf, order] the reflection coefficients k_1..k_p, hop, order, fs, length), Nf = (len(s) - 1) // hop + 1.
    Reflection coefficients, not the polynomial, are the stored form: a blend of two stable sets is stable."""
    e, fs, hop, order = check_noise_analysis_arguments(s, s_recon, fs, order, hop)
    torch, c, dev = _device(device_index)
    L = len(e)
    Nf = (L - 1) // hop + 1
    e_d = torch.as_tensor(np.ascontiguousarray(e), device=dev)
    sigma = torch.empty(Nf, dtype=torch.float64, device=dev)
    refl = torch.empty((Nf, order), dtype=torch.float64, device=dev)
    c.noise_analyse(e_d, L, hop, order, sigma, refl)
    return dict(sigma=sigma.cpu().numpy(), refl=refl.cpu().numpy(), hop=hop, order=order, fs=fs, length=L)


def _device_mod(torch, dev, nz, theta, nu):
    """The optional group of eaqhm_noise_synth on the device: (mod, harmonics, theta, nu)."""
    mod_d, th_d, nu_d = (torch.as_tensor(x, device=dev) for x in (nz["mod"], theta, nu))
    return mod_d, nz["mod_harmonics"], th_d, nu_d


def eaQHMNoiseSynthesis(noise, tau, L_out, seed=0, fundamental=None, *, device_index=0, _ranges=None):
    """Synthesises L_out samples of noise from a model of eaQHMNoiseAnalysis: white noise, a pure
    function of `seed` (0 <= seed < 2**64) and the sample index, through the all-pole lattice of each output frame and
    cross-faded between frames.  `tau[q]`, one value per output frame q = 0 .. (L_out - 1) // hop, is the position (in
    samples of the analysed signal, finite and >= 0) the output sample q hop maps back to: noise_time_map(hop, L_out,
    rho) for a time scale, noise_time_map_contour for a contour; sigma and the reflection coefficients are interpolated
    linearly between the model's frames there.

    `fundamental=(theta, nu)`, one value each per output frame (noise_fundamental gives them), turns the
    pitch-synchronous modulation on: theta[q] is the phase of the output's fundamental in cycles at
    sample q hop, nu[q] its advance in cycles per sample; frame q's samples are multiplied by
    g_q(n') = sqrt(max(0.01, 1 + 2 Re sum_j c_{q,j} exp(2 pi i j (theta[q] + nu[q] (n' - q hop))))).  It needs a model
    with `mod` (eaQHMNoiseModulation).  Without it nothing changes, whatever the model holds.

    `_ranges` (tests): a list of (t_lo, t_hi) output ranges computed one after the other into the same buffer.
    Returns float64[L_out]."""
    nz, tau, L_out, seed = check_noise_synthesis_arguments(noise, tau, L_out, seed)
    fund = check_noise_fundamental(nz, fundamental, len(tau))
    torch, c, dev = _device(device_index)
    sigma_d, refl_d, tau_d = (torch.as_tensor(x, device=dev) for x in (nz["sigma"], nz["refl"], tau))
    out = torch.empty(L_out, dtype=torch.float64, device=dev)
    mod_d = None if fund is None else _device_mod(torch, dev, nz, *fund)
    for t_lo, t_hi in ([(0, L_out)] if _ranges is None else _ranges):
        c.noise_synth(sigma_d, refl_d, len(nz["sigma"]), nz["hop"], nz["order"], tau_d, len(tau), seed, L_out,
                      int(t_lo), int(t_hi), out, mod=mod_d)
    return out.cpu().numpy()


# ---- the formant warp of the noise model
def check_noise_formant(noise_formant, noise, preserve_envelope):
    """Validates eaQHMSynthesis's noise_formant (no device work): a bool; True needs a noise model and the envelope."""
    if not isinstance(noise_formant, (bool, np.bool_)):
        raise ValueError("noise_formant must be True or False, got %r" % (noise_formant,))
    if noise_formant and noise is None:
        raise ValueError("noise_formant=True needs noise=: there is no noise model to warp")
    if noise_formant and not preserve_envelope:
        raise ValueError("noise_formant=True needs preserve_envelope=True, as formant_scale does")
    return bool(noise_formant)


def _frame_alpha(nz, ti, alpha):
    """alpha per noise frame from alpha per analysis instant: linear at sample m hop over the instants ti, flat
    outside them."""
    Nf = len(nz["sigma"])
    return np.interp(np.arange(Nf, dtype=np.float64) * float(nz["hop"]), np.asarray(ti, dtype=np.float64), alpha)


def _frame_rows(nz, ti, f_out):
    """f_out per noise frame from f_out per analysis instant ([No_ti, B] -> [Nf, B]): every column as _frame_alpha
    takes alpha.  A convex combination of valid rows is a valid row; a constant column comes back exactly."""
    return np.ascontiguousarray(np.stack([_frame_alpha(nz, ti, col) for col in f_out.T], axis=1))


def _warp_normalised(f_in, f_out, fs):
    """The breakpoints in cycles per sample, as eaqhm_noise_warp_map and eaqhm_noise_envelope_map take them.  A row
    that equals f_in bit for bit still does."""
    return np.ascontiguousarray(f_in / fs), np.ascontiguousarray(f_out / fs)


def noise_formant_warp(noise, DetComponents, formant_warp):
    """The formant warp of every frame of a noise model, for eaQHMNoiseWarp's `formant_warp` (host only; DESIGN.md
    §10.3): `formant_warp` = (f_in, f_out) is what eaQHMSynthesis takes, f_out [B] or one row per analysis instant;
    frame m takes, column by column, the linear interpolation at sample m hop over the instants' sample positions, flat
    before the first and after the last.  Returns (f_in float64[B], f_out float64[Nf, B]) in Hz."""
    nz = check_noise_model(noise)
    ti = unpack_model(DetComponents)["ti"]
    f_in, f_out = _warp_rows(formant_warp, len(ti), "analysis instant")
    return f_in, _frame_rows(nz, ti, f_out)


def check_noise_warp_map_arguments(noise, formant_warp, formant_scale=1.0):
    """Validates eaQHMNoiseWarp's and noise_envelope's `formant_warp` (no device work): (f_in, f_out) in Hz with f_out
    [B] or [Nf, B], under the rules of check_formant_warp; it excludes a formant_scale != 1.  Returns (model, f_in / fs
    float64[B], f_out / fs float64[Nf, B])."""
    nz = check_noise_model(noise)
    _warp_excludes_scale(formant_scale)
    f_in, f_out = _warp_rows(formant_warp, len(nz["sigma"]), "noise frame")
    return (nz,) + _warp_normalised(f_in, f_out, nz["fs"])


def _device_noise_warp_map(c, sigma_d, refl_d, order, x, y):
    """eaqhm_noise_warp_map on device tensors: (sigma', refl') as new tensors; x [B], y [Nf, B] in cycles per sample."""
    import torch
    x_d, y_d = (torch.as_tensor(v, device=c.device) for v in (x, y))
    sigma_o, refl_o = torch.empty_like(sigma_d), torch.empty_like(refl_d)
    c.noise_warp_map(sigma_d, refl_d, sigma_d.shape[0], order, x_d, y_d, len(x), sigma_o, refl_o)
    return sigma_o, refl_o


def noise_formant_contour(noise, DetComponents, formant_scale):
    """The formant scale of every frame of a noise model, for eaQHMNoiseWarp (host only): `formant_scale` is a number
    or one value per analysis instant of the model (what eaQHMSynthesis takes); frame m takes the linear interpolation
    at sample m hop over the instants' sample positions unpack_model(...)["ti"], flat before the first and after the
    last.  Returns float64[Nf]."""
    nz = check_noise_model(noise)
    ti = unpack_model(DetComponents)["ti"]
    return _frame_alpha(nz, ti, _contour(formant_scale, "formant_scale", len(ti)))


def check_noise_warp_arguments(noise, formant_scale):
    """Validates everything eaQHMNoiseWarp gets (no device work): returns (model, alpha float64[Nf]); formant_scale is
    a number or one value per noise frame, finite and in SCALE_RANGE."""
    nz = check_noise_model(noise)
    Nf = len(nz["sigma"])
    if not _is_contour(formant_scale):
        return nz, np.full(Nf, _scale(formant_scale, "formant_scale"))
    v = _numeric_1d(formant_scale, "formant_scale")
    if len(v) != Nf:
        raise ValueError("formant_scale must have one value per noise frame (%d), got %d" % (Nf, len(v)))
    return nz, np.ascontiguousarray(_in_range(v, "formant_scale"))


def check_noise_envelope_arguments(noise, fs, freqs, formant_scale):
    """Validates everything noise_envelope gets (no device work): returns (model, alpha float64[Nf], fnorm float64[F])
    with fnorm = freqs / fs.  fs must be the model's."""
    fs = _sample_rate(fs)
    f = _freq_grid(freqs)
    nz, alpha = check_noise_warp_arguments(noise, formant_scale)
    if nz["fs"] != fs:
        raise ValueError("the noise model has fs %g, this call %g" % (nz["fs"], fs))
    return nz, alpha, np.ascontiguousarray(f / fs)


def _device_noise_warp(c, sigma_d, refl_d, order, alpha):
    """eaqhm_noise_warp on device tensors: (sigma', refl') as new tensors."""
    import torch
    alpha_d = torch.as_tensor(np.ascontiguousarray(alpha, dtype=np.float64), device=c.device)
    sigma_o, refl_o = torch.empty_like(sigma_d), torch.empty_like(refl_d)
    c.noise_warp(sigma_d, refl_d, sigma_d.shape[0], order, alpha_d, sigma_o, refl_o)
    return sigma_o, refl_o


def eaQHMNoiseWarp(noise, formant_scale=1.0, *, formant_warp=None, device_index=0):
    """The noise model whose spectral envelope is `noise`'s moved up in frequency by `formant_scale` (alpha; DESIGN.md
    §10.1): a feature at F sits at alpha F.  Each frame's all-pole power spectrum sigma^2 / |A|^2 is read at w / alpha on
    a 1025-point grid (held at its Nyquist value above alpha pi), turned into an autocorrelation and re-fitted with the
    analysis's Levinson-Durbin recursion at the same order.  `formant_scale` is a number or one value per noise frame
    (noise_formant_contour gives them from a per-instant contour), finite and in [0.25, 4].  A frame with alpha == 1
    comes back bit for bit, a silent frame silent.  The total power is not renormalised.

    `formant_warp` = (f_in, f_out) in Hz, f_out [B] or one row per noise frame (noise_formant_warp gives them from a map
    per instant), moves the envelope along the piecewise-linear map W of eaQHMSynthesis's `formant_warp` instead (§10.3):
    the spectrum is read at W^-1, held at its Nyquist value where W^-1 passes fs/2.  A frame whose row equals f_in comes
    back bit for bit.  It excludes a formant_scale != 1.

    Returns a new dict(sigma, refl, hop, order, fs, length) of the same layout."""
    if formant_warp is not None:
        nz, x, y = check_noise_warp_map_arguments(noise, formant_warp, formant_scale)
    else:
        nz, alpha = check_noise_warp_arguments(noise, formant_scale)
    torch, c, dev = _device(device_index)
    sigma_d, refl_d = (torch.as_tensor(x_, device=dev) for x_ in (nz["sigma"], nz["refl"]))
    if formant_warp is not None:
        sigma_o, refl_o = _device_noise_warp_map(c, sigma_d, refl_d, nz["order"], x, y)
    else:
        sigma_o, refl_o = _device_noise_warp(c, sigma_d, refl_d, nz["order"], alpha)
    return dict(nz, sigma=sigma_o.cpu().numpy(), refl=refl_o.cpu().numpy())


def noise_envelope(noise, fs, freqs, formant_scale=1.0, *, formant_warp=None, device_index=0):
    """The log power spectrum of every frame of a noise model on a frequency grid, read at the formant scale alpha
    (DESIGN.md §10.1): out[m, t] = 2 ln sigma_m - 2 ln |A_m(e^{jw})| at w = 2 pi min(freqs[t] / alpha_m, fs / 2) / fs,
    the natural log of the power; rows of silent frames are -inf.  It is the exact warped spectrum, the one
    eaQHMNoiseWarp's refit approximates; the counterpart of model_envelope for the noise.  `freqs` (Hz) is 1-D, finite
    and >= 0; `formant_scale` a number or one value per noise frame in [0.25, 4]; `fs` must be the model's.

    With `formant_warp` = (f_in, f_out) (eaQHMNoiseWarp's; §10.3) the read angle is w = min(2 pi W_m^-1(freqs[t]) / fs,
    pi) instead; it excludes a formant_scale != 1.

    Returns float64[Nf, len(freqs)]."""
    nz, alpha, fnorm = check_noise_envelope_arguments(noise, fs, freqs, formant_scale)
    wmap = None if formant_warp is None else check_noise_warp_map_arguments(nz, formant_warp, formant_scale)[1:]
    torch, c, dev = _device(device_index)
    sigma_d, refl_d, f_d = (torch.as_tensor(x, device=dev) for x in (nz["sigma"], nz["refl"], fnorm))
    Nf = len(nz["sigma"])
    out = torch.empty((Nf, len(fnorm)), dtype=torch.float64, device=dev)
    if wmap is None:
        c.noise_envelope(sigma_d, refl_d, Nf, nz["order"], torch.as_tensor(alpha, device=dev), f_d, len(fnorm), out)
    else:
        x_d, y_d = (torch.as_tensor(v, device=dev) for v in wmap)
        c.noise_envelope_map(sigma_d, refl_d, Nf, nz["order"], x_d, y_d, len(wmap[0]), f_d, len(fnorm), out)
    return out.cpu().numpy()


# ---- the noise model to and from cepstral rows
NOISE_CEPSTRUM_EXP_MAX = 600.0   # 4 sum_q |c_q| at most: exp(2 (C - c_0)) stays in the normal range of a double
NOISE_CEPSTRUM_LEVEL_MAX = 700.0  # c_0 + 2 sum_q |c_q| at most: sigma = exp(c_0) sqrt(E) stays finite


def check_noise_cepstrum_arguments(noise, order=63):
    """Validates everything noise_cepstrum gets (no device work): returns (model, Q) with Q = order in [1, 63]."""
    return check_noise_model(noise), _cepstrum_order(order)


def noise_cepstrum(noise, order=63, *, device_index=0):
    """The noise model in cepstral rows: row m holds c_0..c_Q, Q = `order` in [1, 63] (independent of
    the model's LPC order), of C_m(w) = ln(sigma_m / |A_m(e^{jw})|) = c_0 + 2 sum_q c_q cos(q w): the natural log of an
    amplitude in model_cepstrum's layout, so cepstrum_envelope, warp_rows and model_align take the rows unchanged.
    c_0 = ln sigma and c_q = h_q / 2 from the LPC-to-cepstrum recursion: the exact cepstrum of the all-pole frame cut
    at Q, which is the best cosine approximation of that order in the mean square; nothing is fitted, there is no
    lambda.  2 * cepstrum_envelope(rows, fs, f) is noise_envelope(noise, fs, f) up to the cut's remainder.  A silent
    frame (sigma == 0) gives (-inf, 0, .., 0).  The level is that of a spectral density per sample (sigma is the
    standard deviation of the white excitation): it is not comparable to the level of model_cepstrum's harmonic
    envelope.  Returns float64[Nf, Q + 1]."""
    nz, Q = check_noise_cepstrum_arguments(noise, order)
    torch, c, dev = _device(device_index)
    sigma_d, refl_d = (torch.as_tensor(x, device=dev) for x in (nz["sigma"], nz["refl"]))
    Nf = len(nz["sigma"])
    ceps = torch.empty((Nf, Q + 1), dtype=torch.float64, device=dev)
    c.noise_cepstrum(sigma_d, refl_d, Nf, nz["order"], Q, ceps)
    return ceps.cpu().numpy()


def check_noise_from_cepstrum_arguments(ceps, hop, fs, order=None, length=None, mod=None, mod_harmonics=None):
    """Validates everything noise_from_cepstrum gets (no device work): returns (rows float64[Nf, Q + 1], the model's
    other entries as a dict: hop, order, fs, length and, when given, mod and mod_harmonics).  `order` defaults to
    min(63, 2 + round(fs / 1000)), `length` to (Nf - 1) * hop + 1 and must give Nf = (length - 1) // hop + 1 rows.  A row
    that is not empty needs 4 sum_{q>=1} |c_q| <= 600 and c_0 + 2 sum_{q>=1} |c_q| <= 700."""
    C = _cepstrum_rows(ceps, "ceps")
    fs = _sample_rate(fs)
    hop = _integer(hop, "hop")
    order = min(NOISE_MAX_ORDER, 2 + int(round(fs / 1000.0))) if order is None else _integer(order, "order")
    _noise_shape(hop, order)
    Nf = len(C)
    length = (Nf - 1) * hop + 1 if length is None else _integer(length, "length")
    if length < 1 or (length - 1) // hop + 1 != Nf:
        raise ValueError("%d rows at hop %d need (length - 1) // hop + 1 == %d, got length %d" % (Nf, hop, Nf, length))
    live = ~np.isneginf(C[:, 0])
    swing = 2.0 * np.abs(C[:, 1:]).sum(axis=1)
    if np.any(2.0 * swing[live] > NOISE_CEPSTRUM_EXP_MAX):
        raise ValueError("row %d: 4 sum |c_q| must be <= %g, the spectrum's exp would leave the range of a double"
                         % (int(np.flatnonzero(live & (2.0 * swing > NOISE_CEPSTRUM_EXP_MAX))[0]),
                            NOISE_CEPSTRUM_EXP_MAX))
    if np.any(C[live, 0] + swing[live] > NOISE_CEPSTRUM_LEVEL_MAX):
        raise ValueError("c_0 + 2 sum |c_q| must be <= %g: sigma would not be finite" % NOISE_CEPSTRUM_LEVEL_MAX)
    extra = {}
    if mod is not None or mod_harmonics is not None:
        if mod is None or mod_harmonics is None:
            raise ValueError("mod and mod_harmonics come together")
        extra = dict(mod=mod, mod_harmonics=mod_harmonics)
    shell = check_noise_model(dict(sigma=np.zeros(Nf), refl=np.zeros((Nf, order)), hop=hop, order=order, fs=fs,
                                   length=length, **extra))
    del shell["sigma"], shell["refl"]
    return C, shell


def noise_from_cepstrum(ceps, hop, fs, *, order=None, length=None, mod=None, mod_harmonics=None, cep_warp=0.0,
                        device_index=0):
    """A noise model from cepstral rows, the way back from noise_cepstrum: `ceps` float64[Nf, Q + 1]
    holds one row per noise frame (noise_cepstrum's, or rows blended, aligned or built by the caller), frames `hop`
    samples apart.  Per row the power spectrum P[t] = exp(2 (C(w_t) - c_0)) is taken on eaQHMNoiseWarp's 1025-point
    grid, turned into an autocorrelation and fitted by the analysis's Levinson-Durbin recursion at `order` (default
    min(63, 2 + round(fs / 1000)), eaQHMNoiseAnalysis's); sigma = exp(c_0) sqrt(E).  c_0 is kept out of the exponent:
    the reflection coefficients do not depend on column 0 bit for bit, adding d to it multiplies sigma by e^d, and the
    level cannot overflow the grid sums.  A row (-inf, 0, .., 0) gives a silent frame.  `length` (default
    (Nf - 1) * hop + 1) must give Nf = (length - 1) // hop + 1; `mod` / `mod_harmonics` (eaQHMNoiseModulation's) are
    copied into the model under check_noise_model's rules.  A row needs 4 sum_{q>=1} |c_q| <= 600.  `cep_warp` = a,
    |a| <= 0.9, reads rows that lie on the all-pass warped axis (§9.8): P[t] = exp(4 sum_q c_q cos(q Omega_a(w_t))) on the
    same grid; noise_cepstrum's rows are on the linear axis and get there by cepstrum_rewarp(rows, 0, a).

    Returns dict(sigma, refl, hop, order, fs, length[, mod, mod_harmonics]), a model eaQHMNoiseSynthesis,
    eaQHMNoiseWarp and eaQHMSynthesis(noise=) take."""
    C, shell = check_noise_from_cepstrum_arguments(ceps, hop, fs, order, length, mod, mod_harmonics)
    axis = check_cepstrum_warp(cep_warp)
    torch, c, dev = _device(device_index)
    Nf, Q, p = len(C), C.shape[1] - 1, shell["order"]
    sigma = torch.empty(Nf, dtype=torch.float64, device=dev)
    refl = torch.empty((Nf, p), dtype=torch.float64, device=dev)
    _on_axis(c, "noise_from_cepstrum", axis)(torch.as_tensor(C, device=dev), Nf, Q, p, sigma, refl)
    return check_noise_model(dict(shell, sigma=sigma.cpu().numpy(), refl=refl.cpu().numpy()))


def noise_alignment_index(idx, detA, noiseA, detB, noiseB):
    """An alignment of two models' instants carried over to their noise frames (host only).  `idx` is
    alignment_index's output, B's (fractional) instant per instant of A.  Noise frame m of A sits at sample m hopA: its
    fractional position among A's instants (held past the last one) reads `idx` by linear interpolation, B's instants
    turn that into a sample position of B, and the position over hopB, clipped to [0, NfB - 1], is the (fractional)
    frame of B.  The instants of a model are equally spaced, so the two interpolations are one: np.interp over A's
    instants of the B sample positions idx maps them to, which returns arange(Nf) exactly for idx = arange(n), the same
    instants and equal hops.  Both models need the same fs.  Returns float64[NfA]:
    noise_from_cepstrum(warp_rows(noise_cepstrum(noiseB), j), noiseA["hop"], fs, length=noiseA["length"]) is B's noise at
    A's timing."""
    nzA, nzB = check_noise_model(noiseA), check_noise_model(noiseB)
    if nzA["fs"] != nzB["fs"]:
        raise ValueError("the two noise models have different fs: %g and %g" % (nzA["fs"], nzB["fs"]))
    tiA = unpack_model(detA)["ti"].astype(np.float64)
    tiB = unpack_model(detB)["ti"].astype(np.float64)
    t = _numeric_1d(idx, "idx")
    if len(t) != len(tiA):
        raise ValueError("idx must have one value per analysis instant of A (%d), got %d" % (len(tiA), len(t)))
    if not np.all(np.isfinite(t)):
        raise ValueError("idx must be finite")
    at_instants = np.interp(t, np.arange(len(tiB), dtype=np.float64), tiB)     # B's sample position per instant of A
    pos = np.arange(len(nzA["sigma"]), dtype=np.float64) * float(nzA["hop"])
    return np.clip(np.interp(pos, tiA, at_instants) / float(nzB["hop"]), 0.0, len(nzB["sigma"]) - 1.0)


# ---- pitch-synchronous modulation of the noise
def _mod_harmonics(M, name="harmonics"):
    M = _integer(M, name)
    if not 1 <= M <= NOISE_MOD_MAX:
        raise ValueError("%s must be in [1, %d], got %d" % (name, NOISE_MOD_MAX, M))
    return M


def _frac(x):
    """x - floor(x), in [0, 1): a negative x so small that the difference rounds to 1 gives 0."""
    y = x - np.floor(x)
    return np.where(y >= 1.0, 0.0, y)


def _records_phase(rec, K, f0, step, fs):
    """Theta of DESIGN.md §10.2 from records: frac(ph / 2 pi) of slot 0 where it is active (an anchored instant); the
    others by Theta_i = frac(Theta_{i-1} + (step / fs) (f0_{i-1} + f0_i) / 2) in increasing i, those ahead of the first
    anchored instant by the same step backwards from it; from Theta_0 = 0 without any anchored instant."""
    n = len(rec)
    anchored = (rec[:, 0] != 0) & (rec[:, K] > 0) if K else np.zeros(n, dtype=bool)
    th = np.zeros(n)
    if K:
        th[anchored] = _frac(rec[anchored, 2 * K] / (2 * np.pi))
    inc = ((float(step) / float(fs)) * (f0[:-1] + f0[1:]) / 2).tolist()
    first = int(np.flatnonzero(anchored)[0]) if anchored.any() else 0
    v = th.tolist()
    for i in range(first + 1, n):
        if not anchored[i]:
            v[i] = float(_frac(v[i - 1] + inc[i - 1]))
    for i in range(first - 1, -1, -1):
        v[i] = float(_frac(v[i + 1] - inc[i]))
    return np.array(v)


def model_phase(DetComponents, fs, f0=None):
    """The phase of the model's fundamental in cycles, in [0, 1), per analysis instant: the analysed
    phase of slot 0 (harmonic 1) where that slot is active, carried over the other instants by the integral of the
    fundamental `f0` (model_f0(DetComponents, fs), or Hz per instant, finite and > 0 as for phase="shape").  It is what
    the pitch-synchronous envelope of the noise is measured against.  Returns float64[No_ti]."""
    fs = _sample_rate(fs)
    model = unpack_model(DetComponents)
    _, f0 = check_phase_arguments(model, "shape", f0)
    return _records_phase(model["records"], model["Kmax"], f0, model["step"], fs)


def _phase_at(x, theta, f0, ti0, step, fs):
    """Theta(x) = Theta_i + f0_i (x - ti_i) / fs at the instant i nearest to x (rint, clipped to the model)."""
    i = np.clip(np.rint((x - float(ti0)) / float(step)), 0, len(theta) - 1).astype(np.int64)
    return theta[i] + f0[i] * (x - (float(ti0) + i * float(step))) / fs


def _scalar_path(n, rho, beta):
    """(gain, rate, g past the last knot) of the scalar path, in the form of the contour path's."""
    return np.full(n - 1, beta * rho), np.full(n, rho), beta * rho


def _fundamental_at(model, fs, tau, f0, gain, rate, g_last):
    """(theta, nu) of DESIGN.md §10.2 at the input positions tau: tau lies in interval j = min(floor(tau / D), n-1) of
    the instants at offset r = tau - j D; s is §11's advance there (f0 and the rate held past the last instant);
    theta = frac(Theta(tau) + s), nu = (g_j / rho_j) F(tau) / fs with F the linear interpolation of f0."""
    rec, K, D, ti = model["records"], model["Kmax"], float(model["step"]), model["ti"]
    n = len(ti)
    tau = np.asarray(tau, dtype=np.float64)
    S = fundamental_advance(f0, gain, D, fs)
    j = np.clip(np.floor(tau / D).astype(np.int64), 0, n - 1)
    r = tau - j * D
    inside = j <= n - 2
    jc = np.minimum(j, n - 2)
    fa = f0[j]
    fb = np.where(inside, f0[jc + 1], f0[n - 1])
    g = np.where(inside, np.asarray(gain, dtype=np.float64)[jc], g_last)
    s = S[j] + (g - 1.0) * (fa * r + (fb - fa) * r * r / (2.0 * D)) / fs
    Theta = _phase_at(tau, _records_phase(rec, K, f0, D, fs), f0, ti[0], D, fs)
    F = np.interp(tau, ti.astype(np.float64), f0)
    return np.ascontiguousarray(_frac(Theta + s)), np.ascontiguousarray((g / np.asarray(rate, dtype=np.float64)[j]) * F / fs)


def _tau(tau):
    tau = _numeric_1d(tau, "tau")
    if len(tau) == 0 or not np.all(np.isfinite(tau)) or np.any(tau < 0):
        raise ValueError("tau must be non-empty, finite and >= 0")
    return tau


def noise_fundamental(DetComponents, fs, tau, time_map=None, time_scale=1.0, pitch_scale=1.0, f0=None):
    """The fundamental the synthesis plays at the output frames of the noise (host only): for
    `tau` (noise_time_map / noise_time_map_contour) returns (theta, nu), float64 per output frame: the phase of the
    fundamental in cycles, in [0, 1), at the frame's centre and its advance in cycles per output sample.  It is the
    fundamental of phase="shape" (§11): the model's phase at tau plus the advance s.  The scalar path takes the numbers
    `time_scale` and `pitch_scale`; the contour path takes `time_map` = contour_time_map(rho, beta, step, length) and
    `pitch_scale` = beta (its value at the last instant holds past it; `time_scale` is in the map).  `f0` as for
    phase="shape"; default model_f0.  This is eaQHMNoiseSynthesis's `fundamental`."""
    fs = _sample_rate(fs)
    model = unpack_model(DetComponents)
    _check_records(model)
    _, f0 = check_phase_arguments(model, "shape", f0)
    tau = _tau(tau)
    n = len(model["ti"])
    if time_map is None:
        path = _scalar_path(n, _scale(time_scale, "time_scale"), _scale(pitch_scale, "pitch_scale"))
    else:
        try:
            gain, rate = _numeric_1d(time_map["gain"], "time_map gain"), _numeric_1d(time_map["rate"], "time_map rate")
        except (TypeError, KeyError, IndexError):
            raise ValueError("time_map is the dict contour_time_map returns") from None
        if len(gain) != n - 1 or len(rate) != n or not np.all(np.isfinite(gain)) or not np.all(rate > 0):
            raise ValueError("time_map is of another model: gain must have %d values and rate %d (> 0)" % (n - 1, n))
        path = (gain, rate, rate[-1] * _contour(pitch_scale, "pitch_scale", n)[-1])
    return _fundamental_at(model, fs, tau, f0, *path)


def check_noise_fundamental(nz, fundamental, Nq):
    """Validates eaQHMNoiseSynthesis's `fundamental` (no device work): None, or (theta, nu) as two contiguous
    float64[Nq], finite; it needs a checked model `nz` with mod."""
    if fundamental is None:
        return None
    if "mod" not in nz:
        raise ValueError("fundamental= needs a noise model with mod (eaQHMNoiseModulation)")
    try:
        theta, nu = fundamental
    except (TypeError, ValueError):
        raise ValueError("fundamental must be the pair (theta, nu) of noise_fundamental") from None
    theta, nu = _numeric_1d(theta, "theta"), _numeric_1d(nu, "nu")
    if len(theta) != Nq or len(nu) != Nq:
        raise ValueError("theta and nu must have one value per output frame (%d), got %d and %d"
                         % (Nq, len(theta), len(nu)))
    if not (np.all(np.isfinite(theta)) and np.all(np.isfinite(nu))):
        raise ValueError("theta and nu must be finite")
    return np.ascontiguousarray(theta), np.ascontiguousarray(nu)


def check_noise_modulation(noise_modulation, nz):
    """Validates eaQHMSynthesis's noise_modulation (no device work): a bool; True needs a noise model with mod."""
    if not isinstance(noise_modulation, (bool, np.bool_)):
        raise ValueError("noise_modulation must be True or False, got %r" % (noise_modulation,))
    if noise_modulation and nz is None:
        raise ValueError("noise_modulation=True needs noise=: there is no noise to modulate")
    if noise_modulation and "mod" not in nz:
        raise ValueError("noise_modulation=True needs a noise model with mod (eaQHMNoiseModulation)")
    return bool(noise_modulation)


def check_noise_modulation_arguments(s, s_recon, noise, DetComponents, harmonics=2, f0=None):
    """Validates everything eaQHMNoiseModulation gets (no device work): returns (e, model of the noise, unpacked model,
    M, f0).  The noise model and the deterministic model must be of this signal: the length is s's, and no instant lies
    past it."""
    nz = check_noise_model(noise)
    a, b = _signal_pair(s, s_recon)
    if len(a) != nz["length"]:
        raise ValueError("the noise model is of another signal: length %d, s has %d" % (nz["length"], len(a)))
    M = _mod_harmonics(harmonics)
    model = unpack_model(DetComponents)
    if int(model["ti"][-1]) >= len(a):
        raise ValueError("the model is of another signal: its last instant (%d) lies past s (%d samples)"
                         % (int(model["ti"][-1]), len(a)))
    if not np.all(np.isfinite(model["records"])):
        raise ValueError("the model holds non-finite values")
    _, f0 = check_phase_arguments(model, "shape", f0)
    return a - b, nz, model, M, f0


def eaQHMNoiseModulation(s, s_recon, noise, DetComponents, harmonics=2, f0=None, *, device_index=0):
    """The pitch-synchronous modulation of the noise.  In voiced speech the noise comes in bursts
    locked to the glottal cycle; per frame of `noise` (eaQHMNoiseAnalysis of the same `s`, `s_recon`) this measures the
    power of the windowed residual over the phase Theta of the model's fundamental (model_phase(DetComponents, fs, f0))
    as Fourier coefficients c_j = sum u exp(-2 pi i j Theta) / sum u, u = (w e)^2, j = 1..`harmonics` (1 to 8).  They
    stand for the power envelope g^2(theta) = 1 + 2 Re sum_j c_j exp(2 pi i j theta) over one pitch period.  A frame
    without power, and a frame whose nearest analysis instant has no active partial (unvoiced), gets c = 0 exactly.

    Returns a copy of `noise` with mod=float64[Nf, 2 harmonics] (Re c_1, Im c_1, ..) and mod_harmonics=harmonics, which
    eaQHMNoiseSynthesis(fundamental=) and eaQHMSynthesis(noise_modulation=True) play; eaQHMNoiseWarp carries them
    through."""
    e, nz, model, M, f0 = check_noise_modulation_arguments(s, s_recon, noise, DetComponents, harmonics, f0)
    torch, c, dev = _device(device_index)
    rec, K, D, ti = model["records"], model["Kmax"], model["step"], model["ti"]
    theta = _records_phase(rec, K, f0, D, nz["fs"])
    voiced = np.ascontiguousarray((rec[:, :K] != 0).any(axis=1), dtype=np.uint8)
    e_d, th_d, f0_d, v_d = (torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in (e, theta, f0, voiced))
    Nf = len(nz["sigma"])
    mod = torch.empty((Nf, 2 * M), dtype=torch.float64, device=dev)
    c.noise_modulation(e_d, len(e), nz["hop"], th_d, f0_d, v_d, len(ti), float(ti[0]), float(D), nz["fs"], M, mod)
    return dict(nz, mod=mod.cpu().numpy(), mod_harmonics=M)
