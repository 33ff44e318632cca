"""The model as records, and what is read off the records alone: instants, fundamental, phase, the time map of a pair
of contours, and the formant scale and warp rules that need the model's length.

    unpack_model(DetComponents) -> dict(records, step, Kmax, ti, quirk_cells)
    scale_contour(DetComponents, fs, times_s, values) -> float64[No_ti]
    contour_time_map(rho, beta, step, length) -> dict(rate, gain, C, L_out, rate_min)
    check_formant_scale(model, formant_scale, preserve_envelope) -> alpha: float, or float64[No_ti] for a contour
    check_formant_warp(model, fs, formant_warp, formant_scale=1.0, preserve_envelope=True) -> (f_in[B], f_out[No_ti, B])
    formant_warp_vtln(fs, alpha, knee=0.875) -> (f_in, f_out): the two-breakpoint VTLN map
    model_f0(DetComponents, fs) -> float64[No_ti]
    model_phase(DetComponents, fs, f0=None) -> float64[No_ti]
    check_phase_arguments(model, phase, f0) -> (shape: bool, f0: float64[No_ti] or None); PHASE_MODES
    fundamental_advance(f0, gain, step, fs) -> float64[n] in [0, 1)

`DetComponents` is either form eaQHMAnalysisAndSynthesis returns: the list of Deterministic (det_format="structs") or
the dict of arrays (det_format="arrays"), edited or not.  _device gives every module above this one its library
context, from functions._ctx; _device_records puts the records on that device; _agree holds a size the library reports
to the host's own mirror of it.
"""
from itertools import chain, compress, repeat
from operator import itemgetter

import numpy as np

from .args import (SCALE_RANGE, _contour, _is_contour, _numeric_1d, _sample_rate, _scale, _warp_excludes_scale,
                   _warp_rows, check_curve)


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


def _check_records(model):
    rec = model["records"]
    if len(rec) < 4:
        raise ValueError("the model needs at least 4 analysis instants (the cubic interpolation of the tracks)")
    if not np.all(np.isfinite(rec)):
        raise ValueError("the model holds non-finite values")
    if np.any(rec[:, :model["Kmax"]] < 0):
        raise ValueError("amplitudes must be >= 0 (the model holds |a_k|)")


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


def _agree(what, lib_value, host_value):
    """RuntimeError naming `what` unless the library's value is the host mirror's."""
    if lib_value != host_value:
        raise RuntimeError("libeaqhm_hip.so and the host disagree on " + what)


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
