"""Formant tracks: where the formants of a voice are, from the poles of its all-pole envelope, through
libeaqhm_hip.so (eaqhm_allpole_roots, eaqhm_formant_candidates, eaqhm_formant_forward, eaqhm_formant_backtrack).

    allpole_roots(model, *, device_index=0) -> (roots complex128[Nf, p], iters int32[Nf])
    formant_candidates(model, *, fmin=50.0, fmax=5500.0, max_bandwidth=1000.0, device_index=0) -> dict(f, b, count)
    formant_tracks(cand, n_formants=3, reference=(550, 1650, 2750, 3850), *, freq_cost=1.0, bandwidth_cost=1.0,
                   jump_cost=1.0, absent_cost=2.0, device_index=0, return_path=False) -> (F, B) float64[Nf, N]
    formant_states(N) -> int8[C(8 + N, N), N]: the tracker's state table
    formant_cost_tables(cand, N, reference, freq_cost, bandwidth_cost) -> (L float64[T, N, 8], lf float64[T, 8])
    signal_allpole(s, fs, order=None, hop=None, preemphasis=0.97, *, device_index=0) -> an all-pole model of a signal
    model_allpole(DetComponents, fs, order=None, hop=None, *, device_index=0) -> the all-pole fit of a model's envelope
    formant_warp_from_tracks(FA, FB, fs, *, anchor_nyquist=True) -> (f_in, f_out) for eaQHMSynthesis(formant_warp=)

Argument checks without device work: check_allpole_model(model), check_candidate_arguments(model, fmin, fmax,
max_bandwidth), check_candidates(cand), check_track_arguments(cand, n_formants, reference, freq_cost, bandwidth_cost,
jump_cost, absent_cost), check_signal_allpole_arguments(s, fs, order, hop, preemphasis).  Constants: FORMANT_ITMAX,
FORMANT_CANDIDATES, FORMANT_TRACKS_MAX.

This module is reached as eaqhm_amd.formant; the package does not re-export it.  An all-pole model is the dict of
eaQHMNoiseAnalysis and noise_from_cepstrum: sigma[Nf], refl[Nf, p] with |k| < 1, hop, order, fs, length.  There is no
CPU path: without the library or a GPU every function that reaches the device raises.
"""
from itertools import product

import numpy as np

from .args import SCALE_RANGE, _integer, _numeric_1d, _sample_rate, _warp_rows
from .noise import check_noise_analysis_arguments, check_noise_model

FORMANT_ITMAX = 64            # EAQHM_FORMANT_ITMAX: iters = FORMANT_ITMAX + 1 marks a frame that did not finish
FORMANT_CANDIDATES = 8        # EAQHM_FORMANT_CAND
FORMANT_TRACKS_MAX = 4        # EAQHM_FORMANT_TRACKS


def _number(v, name, lo=None):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (name, v)) from None
    if not np.isfinite(v) or (lo is not None and v < lo):
        raise ValueError("%s must be finite%s, got %r" % (name, "" if lo is None else " and >= %g" % lo, v))
    return v


def _device_index(device_index):
    if isinstance(device_index, bool) or not isinstance(device_index, (int, np.integer)) or device_index < 0:
        raise ValueError("device_index must be a non-negative integer, got %r" % (device_index,))
    return int(device_index)


def _track_count(n):
    n = _integer(n, "n_formants")
    if not 1 <= n <= FORMANT_TRACKS_MAX:
        raise ValueError("n_formants must be in [1, %d], got %d" % (FORMANT_TRACKS_MAX, n))
    return n


# ---- the poles
def check_allpole_model(model):
    """check_noise_model (no device work): the all-pole model with refl float64[Nf, p] contiguous, |k| < 1."""
    return check_noise_model(model)


def _roots_on_device(nz, torch, c, dev):
    Nf, p = nz["refl"].shape
    refl = torch.as_tensor(nz["refl"], device=dev)
    roots = torch.empty((Nf, p, 2), dtype=torch.float64, device=dev)
    iters = torch.empty(Nf, dtype=torch.int32, device=dev)
    c.allpole_roots(refl, Nf, p, roots, iters)
    return roots, iters


def allpole_roots(model, *, device_index=0):
    """The poles of every frame of an all-pole model: the roots of P(z) = z^p + a_1 z^(p-1) + .. + a_p,
    a the step-up of the frame's reflection coefficients, by the Aberth-Ehrlich iteration.  Returns (roots
    complex128[Nf, p], iters int32[Nf]).  A frame whose last p - pe coefficients are zero has p - pe roots that are exactly
    0, in its last places; a silent frame has only those.  iters counts the steps; FORMANT_ITMAX + 1 marks a frame that
    did not finish (its last iterate is returned).  Every accepted root satisfies |P(z)| <= 8 pe 2^-53 sum |a_j|
    |z|^(pe-j) in float64."""
    nz = check_allpole_model(model)
    device_index = _device_index(device_index)
    from .records import _device
    torch, c, dev = _device(device_index)
    roots, iters = _roots_on_device(nz, torch, c, dev)
    r = roots.cpu().numpy()
    return r[..., 0] + 1j * r[..., 1], iters.cpu().numpy()


# ---- the candidates
def check_candidate_arguments(model, fmin=50.0, fmax=5500.0, max_bandwidth=1000.0):
    """Validates what formant_candidates gets (no device work): returns (model, fmin, fmax, max_bandwidth) with fmax
    clipped to fs / 2.  0 <= fmin < fmax, max_bandwidth > 0, all finite."""
    nz = check_allpole_model(model)
    fmin = _number(fmin, "fmin", 0)
    fmax = _number(fmax, "fmax", 0)
    max_bandwidth = _number(max_bandwidth, "max_bandwidth", 0)
    fmax = min(fmax, nz["fs"] / 2.0)
    if not fmin < fmax:
        raise ValueError("fmin %g must lie below fmax %g (clipped to fs / 2)" % (fmin, fmax))
    if not max_bandwidth > 0:
        raise ValueError("max_bandwidth must be > 0, got %g" % max_bandwidth)
    return nz, fmin, fmax, max_bandwidth


def formant_candidates(model, *, fmin=50.0, fmax=5500.0, max_bandwidth=1000.0, device_index=0):
    """The formant candidates of every frame: the poles with Im z > 0, frequency f = arg z fs / (2 pi)
    in [fmin, fmax] (fmax clipped to fs / 2) and bandwidth b = -ln|z| fs / pi <= max_bandwidth, in ascending frequency,
    the lowest 8.  Returns dict(f=float64[Nf, 8], b=float64[Nf, 8], count=int32[Nf], hop, fs, unfinished): NaN beyond the
    count; `unfinished` counts the frames whose iteration did not finish (they have no candidates).  The roots stay on
    the device."""
    nz, fmin, fmax, max_bandwidth = check_candidate_arguments(model, fmin, fmax, max_bandwidth)
    device_index = _device_index(device_index)
    from .records import _device
    torch, c, dev = _device(device_index)
    Nf, p = nz["refl"].shape
    roots, iters = _roots_on_device(nz, torch, c, dev)
    f = torch.empty((Nf, FORMANT_CANDIDATES), dtype=torch.float64, device=dev)
    b = torch.empty((Nf, FORMANT_CANDIDATES), dtype=torch.float64, device=dev)
    count = torch.empty(Nf, dtype=torch.int32, device=dev)
    c.formant_candidates(roots, iters, Nf, p, nz["fs"], fmin, fmax, max_bandwidth, f, b, count)
    return dict(f=f.cpu().numpy(), b=b.cpu().numpy(), count=count.cpu().numpy(), hop=nz["hop"], fs=nz["fs"],
                unfinished=int((iters.cpu().numpy() == FORMANT_ITMAX + 1).sum()))


# ---- the tracker
_STATES = {}


def formant_states(N):
    """The tracker's states for N tracks, int8[C(8 + N, N), N]: every tuple that gives each slot a candidate index in
    [0, 8) or -1 (absent) with the used indices strictly increasing along the slots, in lexicographic order of the
    tuples (-1 first): 9, 45, 165, 495 rows."""
    N = _track_count(N)
    if N not in _STATES:
        rows = []
        for s in product(range(-1, FORMANT_CANDIDATES), repeat=N):
            used = [v for v in s if v >= 0]
            if all(x < y for x, y in zip(used, used[1:])):
                rows.append(s)
        table = np.array(rows, dtype=np.int8)
        table.setflags(write=False)
        _STATES[N] = table
    return _STATES[N]


def check_candidates(cand):
    """Validates a candidate set (no device work): a dict with f, b float64[T, 8] and count int32[T] in [0, 8]; within the
    count f is finite and > 0 and b finite.  Returns (f, b, count) contiguous."""
    if not isinstance(cand, dict) or not all(k in cand for k in ("f", "b", "count")):
        raise ValueError("candidates are the dict formant_candidates returns: f, b, count")
    f, b = np.asarray(cand["f"]), np.asarray(cand["b"])
    if f.dtype.kind not in "iuf" or b.dtype.kind not in "iuf" or f.ndim != 2 or f.shape != b.shape \
            or f.shape[1] != FORMANT_CANDIDATES or f.shape[0] < 1:
        raise ValueError("f and b must be (T, %d) arrays of numbers with T >= 1" % FORMANT_CANDIDATES)
    count = np.asarray(cand["count"])
    if count.dtype.kind not in "iu" or count.shape != (f.shape[0],):
        raise ValueError("count must be an integer array with one entry per frame (%d)" % f.shape[0])
    if np.any(count < 0) or np.any(count > FORMANT_CANDIDATES):
        raise ValueError("count must lie in [0, %d]" % FORMANT_CANDIDATES)
    f = np.ascontiguousarray(f, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    used = np.arange(FORMANT_CANDIDATES)[None, :] < count[:, None]
    if not (np.all(np.isfinite(f[used])) and np.all(f[used] > 0) and np.all(np.isfinite(b[used]))):
        raise ValueError("within the count f must be finite and > 0 and b finite")
    return f, b, np.ascontiguousarray(count, dtype=np.int32)


def check_track_arguments(cand, n_formants=3, reference=(550, 1650, 2750, 3850), freq_cost=1.0, bandwidth_cost=1.0,
                          jump_cost=1.0, absent_cost=2.0):
    """Validates everything formant_tracks gets (no device work): returns (f, b, count, N, ref float64[N], freq_cost,
    bandwidth_cost, jump_cost, absent_cost).  1 <= n_formants <= 4; reference holds at least n_formants values, finite,
    positive and strictly increasing (the first n_formants are used); the four costs are finite and >= 0."""
    f, b, count = check_candidates(cand)
    N = _track_count(n_formants)
    ref = _numeric_1d(reference, "reference")
    if len(ref) < N:
        raise ValueError("reference must hold at least n_formants = %d values, got %d" % (N, len(ref)))
    if not np.all(np.isfinite(ref)) or np.any(ref <= 0) or np.any(np.diff(ref) <= 0):
        raise ValueError("reference must be finite, positive and strictly increasing")
    return (f, b, count, N, np.ascontiguousarray(ref[:N], dtype=np.float64), _number(freq_cost, "freq_cost", 0),
            _number(bandwidth_cost, "bandwidth_cost", 0), _number(jump_cost, "jump_cost", 0),
            _number(absent_cost, "absent_cost", 0))


def formant_cost_tables(cand, N, reference, freq_cost=1.0, bandwidth_cost=1.0):
    """The tables the tracker reads, formed on the host with NumPy: L float64[T, N, 8] with
    L[t, n, c] = freq_cost |f_c - ref_n| / 1000 + bandwidth_cost b_c / f_c, and lf float64[T, 8] = log2 f_c; entries
    beyond a frame's count are 0 (they are never looked at)."""
    f, b, count, N, ref, wf, wb, _, _ = check_track_arguments(cand, N, reference, freq_cost, bandwidth_cost)
    used = np.arange(FORMANT_CANDIDATES)[None, :] < count[:, None]
    fu = np.where(used, f, 1.0)
    bu = np.where(used, b, 0.0)
    L = wf * np.abs(fu[:, None, :] - ref[None, :, None]) / 1000.0 + (wb * bu / fu)[:, None, :]
    L = np.where(used[:, None, :], L, 0.0)
    return np.ascontiguousarray(L), np.ascontiguousarray(np.where(used, np.log2(fu), 0.0))


def formant_tracks(cand, n_formants=3, reference=(550, 1650, 2750, 3850), *, freq_cost=1.0, bandwidth_cost=1.0,
                   jump_cost=1.0, absent_cost=2.0, device_index=0, return_path=False):
    """Sorts the candidates of every frame into n_formants tracks F1..FN: a Viterbi decode over the
    states of formant_states(N).  A slot that holds candidate c pays freq_cost |f_c - reference_n| / 1000 +
    bandwidth_cost b_c / f_c, an absent slot pays absent_cost, and from one frame to the next a slot pays jump_cost
    |log2 f' - log2 f| (nothing where it is absent on either side): Praat's costs plus the price of an absent slot.
    Returns (F, B) float64[T, N], NaN where a slot is absent; with return_path=True (F, B, q int32[T], total): the
    state of every frame and the cost of the path.  The same bits on every call."""
    f, b, count, N, ref, wf, wb, wj, ac = check_track_arguments(cand, n_formants, reference, freq_cost, bandwidth_cost,
                                                                jump_cost, absent_cost)
    device_index = _device_index(device_index)
    L, lf = formant_cost_tables(dict(f=f, b=b, count=count), N, ref, wf, wb)
    states = formant_states(N)
    T, S = len(count), len(states)
    from .records import _device
    torch, c, dev = _device(device_index)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    bp = torch.empty((T, S), dtype=torch.int16, device=dev)
    last = torch.empty(S, dtype=torch.float64, device=dev)
    q = torch.empty(T, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    c.formant_forward(up(L), up(lf), up(count), up(np.array(states)), N, T, wj, ac, bp, last)   # the table is read-only
    c.formant_backtrack(bp, last, N, T, q, total)
    q_h = q.cpu().numpy()
    F, B = tracks_from_path(f, b, states, q_h)
    return (F, B, q_h, float(total.cpu().numpy()[0])) if return_path else (F, B)


def tracks_from_path(f, b, states, q):
    """(F, B) float64[T, N] of the state sequence q: the candidate each slot holds, NaN where it is absent."""
    idx = np.asarray(states)[np.asarray(q)].astype(np.int64)            # [T, N]
    rows = np.arange(len(idx))[:, None]
    F = np.where(idx >= 0, np.asarray(f)[rows, np.maximum(idx, 0)], np.nan)
    B = np.where(idx >= 0, np.asarray(b)[rows, np.maximum(idx, 0)], np.nan)
    return F, B


# ---- where the all-pole model comes from
def check_signal_allpole_arguments(s, fs, order=None, hop=None, preemphasis=0.97):
    """Validates what signal_allpole gets (no device work): returns (x, fs, hop, order) with x the pre-emphasised
    signal x[n] = s[n] - preemphasis s[n-1] (x[0] = s[0]); 0 <= preemphasis < 1; s, fs, order and hop under
    check_noise_analysis_arguments' rules."""
    a = _number(preemphasis, "preemphasis", 0)
    if not a < 1:
        raise ValueError("preemphasis must be in [0, 1), got %g" % a)
    s = _numeric_1d(s, "s")
    x, fs, hop, order = check_noise_analysis_arguments(s, np.zeros(len(s)), fs, order, hop)
    y = x.copy()
    y[1:] = x[1:] - a * x[:-1]
    return y, fs, hop, order


def signal_allpole(s, fs, order=None, hop=None, preemphasis=0.97, *, device_index=0):
    """The all-pole (LPC) envelope of every frame of a signal: eaQHMNoiseAnalysis of the pre-emphasised signal against
    zeros.  Returns the model dict(sigma, refl, hop, order, fs, length)."""
    x, fs, hop, order = check_signal_allpole_arguments(s, fs, order, hop, preemphasis)
    from .noise import eaQHMNoiseAnalysis
    return eaQHMNoiseAnalysis(x, np.zeros(len(x)), fs, order, hop, device_index=_device_index(device_index))


def model_allpole(DetComponents, fs, order=None, hop=None, *, device_index=0):
    """The all-pole fit of a model's cepstral envelope: noise_from_cepstrum(model_cepstrum(DetComponents, fs), ..), one
    row per analysis instant, `hop` the model's step unless given."""
    from .cepstrum import model_cepstrum
    from .noise import noise_from_cepstrum
    from .records import unpack_model
    device_index = _device_index(device_index)
    hop = unpack_model(DetComponents)["step"] if hop is None else _integer(hop, "hop")
    ceps = model_cepstrum(DetComponents, fs, device_index=device_index)
    return noise_from_cepstrum(ceps, hop, fs, order=order, device_index=device_index)


# ---- from two voices' tracks to a formant warp
def formant_warp_from_tracks(FA, FB, fs, *, anchor_nyquist=True):
    """The piecewise-linear formant warp that carries speaker A's formants to speaker B's: (f_in,
    f_out) for eaQHMSynthesis(model_of_A, .., formant_warp=).  FA float64[TA, N] and FB float64[TB, N] are formant_tracks'
    F of the two voices.  Slot n gives the breakpoint (median of FA[:, n], median of FB[:, n]), each median over the
    frames where the slot is present; a slot that is absent throughout either track gives none.  With anchor_nyquist
    the point (fs / 2, fs / 2) closes the map where it is admissible: above the last breakpoint on both axes, at a
    slope inside [0.25, 4].  ValueError, naming the slot, where the breakpoints are not strictly increasing or a
    segment's slope (the one from the origin included) leaves [0.25, 4], and where no slot gives a breakpoint."""
    fs = _sample_rate(fs)
    FA, FB = np.asarray(FA), np.asarray(FB)
    if FA.dtype.kind not in "iuf" or FB.dtype.kind not in "iuf" or FA.ndim != 2 or FB.ndim != 2 \
            or FA.shape[1] != FB.shape[1] or not 1 <= FA.shape[1] <= FORMANT_TRACKS_MAX or 0 in (len(FA), len(FB)):
        raise ValueError("FA and FB must be (frames, N) arrays of numbers with the same N in [1, %d]" % FORMANT_TRACKS_MAX)
    FA, FB = FA.astype(np.float64), FB.astype(np.float64)
    if np.isinf(FA).any() or np.isinf(FB).any() or np.nanmin(np.where(np.isnan(FA), 1, FA)) <= 0 \
            or np.nanmin(np.where(np.isnan(FB), 1, FB)) <= 0:
        raise ValueError("formant frequencies must be finite and > 0 (NaN: absent)")
    x, y, slots = [], [], []
    for n in range(FA.shape[1]):
        a, b = FA[~np.isnan(FA[:, n]), n], FB[~np.isnan(FB[:, n]), n]
        if len(a) and len(b):
            x.append(float(np.median(a)))
            y.append(float(np.median(b)))
            slots.append(n)
    if not x:
        raise ValueError("no slot is present in both tracks: there is no breakpoint")
    px = py = 0.0
    for xi, yi, n in zip(x, y, slots):
        if not (xi > px and yi > py):
            raise ValueError("slot %d (F%d): the breakpoint (%g, %g) does not lie above the one before, (%g, %g)"
                             % (n, n + 1, xi, yi, px, py))
        slope = (yi - py) / (xi - px)
        if not SCALE_RANGE[0] <= slope <= SCALE_RANGE[1]:
            raise ValueError("slot %d (F%d): the segment up to (%g, %g) has slope %g, outside [%g, %g]"
                             % (n, n + 1, xi, yi, slope, SCALE_RANGE[0], SCALE_RANGE[1]))
        px, py = xi, yi
    ny = fs / 2.0
    if anchor_nyquist and px < ny and py < ny and SCALE_RANGE[0] <= (ny - py) / (ny - px) <= SCALE_RANGE[1]:
        x.append(ny)
        y.append(ny)
    f_in, f_out = _warp_rows((np.array(x), np.array(y)), 1, "track")
    return f_in, f_out[0]
