"""SWIPE' pitch estimation on the device: swipe.py's algorithm, quirks included, through libeaqhm_hip.so.

    swipep_device(x, fs, plim, *, device_index=0, return_strengths=False) -> float64[T, 3] [time s, pitch Hz, strength]
        (and S float64[len(pc), T] with return_strengths=True): swipe.swipep's layout and 1 ms grid
    swipe_plan(n, fs, plim) -> every small array the kernels need, host only, cached
    analysis_pitch_track(speechFile, gender, fc=0, *, device_index=0) -> the track the analysis would compute for the
        file, ready for pitch_track= / pitch_tracks=[...]
    check_swipe_arguments(x, fs, plim) -> (x float64[n], fs, (lo, hi)): validation, no device work
    swipep_viterbi(x, fs, plim, *, jump_cost=4.0, free_jump=1/48, max_jump=0.5, unvoiced=None, voicing_cost=1.0, ...)
        -> the same layout, the pitch taken along the best CONTINUOUS path through the strengths
    viterbi_costs(npc, jump_cost, free_jump, max_jump) -> the cost of a step of k candidates, float64[W + 1]
    viterbi_track(S, cost, *, unvoiced=None, voicing_cost=1.0) -> (q int32[T], last float64[npc + 1]): the decode alone,
        over any host matrix
    analysis_pitch_track_viterbi(speechFile, gender, fc=0, **options) -> analysis_pitch_track with swipep_viterbi

This module is reached as eaqhm_amd.pitch; the package does not re-export it, and the analysis keeps calling swipe.swipep
unless it is handed a track.

The definition is DESIGN.md §13.  The host forms, with exactly the NumPy expressions of swipe.py, what depends on
(n, fs, plim) alone: the instants, the candidates, the windows, the ERB grid and its interpolation tables, the kernel matrix
of every window size and the refinement tables.  The device does what depends on the signal: per window size the
normalised square-root ERB spectrum of every frame (eaqhm_swipe_loudness), its product with the kernel matrix
(eaqhm_swipe_scores), then per instant the time interpolation, the weighted sum over the window sizes, the first maximum
and the parabolic refinement (eaqhm_swipe_pick).  The pitch is read from a table of the values swipep's scalar power
gives, so equal decisions give equal bits.  There is no CPU path: without the library or a GPU swipep_device raises.
"""
from collections import OrderedDict

import numpy as np

from .swipe import _primes_with_one, erbs2hz, hz2erbs

SWIPE_WINDOW_MAX = 8192        # EAQHM_SWIPE_WMAX
SWIPE_ERB_MAX = 1024           # EAQHM_SWIPE_EMAX
SWIPE_WINDOWS_MAX = 8          # EAQHM_SWIPE_WINDOWS
SWIPE_FINE_MAX = 64            # EAQHM_SWIPE_FINE
VITERBI_TILE = 8               # EAQHM_VITERBI_TILE
VITERBI_NPC_MAX = 1024         # EAQHM_VITERBI_NPC
VITERBI_JUMP_MAX = 256         # EAQHM_VITERBI_JUMP
_PLANS, _KERNELS, _DEVICE_PLANS = OrderedDict(), OrderedDict(), OrderedDict()
_CACHED = 8                    # plans, kernel matrices and device copies kept


def _remember(cache, key, value):
    cache[key] = value
    while len(cache) > _CACHED:
        cache.popitem(last=False)
    return value


def _limits(fs, plim):
    try:
        fs = float(fs)
        lo, hi = (float(v) for v in plim)
    except (TypeError, ValueError):
        raise ValueError("fs must be a number and plim two numbers") from None
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError("fs must be positive, got %r" % (fs,))
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo < hi <= fs / 2):
        raise ValueError("plim must be two finite values with 0 < plim[0] < plim[1] <= fs / 2, got %r" % (tuple(plim),))
    return fs, lo, hi


def _grid(fs, plim):
    """swipe.py:90-99 without the signal: (log2pc, pc, ws, pO, d, fERBs)."""
    log2pc = np.arange(np.log2(plim[0]), np.log2(plim[-1]), 1.0 / 96.0)
    pc = np.power(2, log2pc)
    logWs = np.round(np.log2(8 * (float(fs) / np.asarray(plim, dtype=np.float64))))
    ws = np.power(2, np.arange(logWs[0], logWs[1] - 1, -1))
    pO = 8 * fs / ws
    d = 1 + log2pc - np.log2(8 * (fs / ws[0]))
    fERBs = erbs2hz(np.arange(hz2erbs(pc[0] / 4), hz2erbs(fs / 2), 0.1))
    return log2pc, pc, ws, pO, d, fERBs


def _check_grid(fs, lo, hi):
    grid = _grid(fs, [lo, hi])
    pc, ws, fERBs = grid[1], grid[2], grid[5]
    if len(pc) < 3:
        raise ValueError("plim [%g, %g] gives %d pitch candidates, at least 3 are needed" % (lo, hi, len(pc)))
    if ws[0] > SWIPE_WINDOW_MAX:
        raise ValueError("the largest window has %d samples, the limit is %d: plim[0] above %.6g Hz fits at fs = %g"
                         % (ws[0], SWIPE_WINDOW_MAX, 8 * fs / 2 ** (np.log2(SWIPE_WINDOW_MAX) + 0.5), fs))
    if len(ws) > SWIPE_WINDOWS_MAX:
        raise ValueError("plim [%g, %g] needs %d window sizes, the limit is %d" % (lo, hi, len(ws), SWIPE_WINDOWS_MAX))
    if len(fERBs) > SWIPE_ERB_MAX:
        raise ValueError("fs = %g and plim[0] = %g give %d ERB points, the limit is %d" % (fs, lo, len(fERBs), SWIPE_ERB_MAX))
    return grid


def check_swipe_arguments(x, fs, plim):
    """Validates what swipep_device gets (no device work): returns (x float64[n], fs, (plim[0], plim[1])).  ValueError for
    x not 1-D, empty or not finite; fs <= 0; plim not two finite values with 0 < plim[0] < plim[1] <= fs / 2; fewer than 3
    pitch candidates; a largest window above 8192 samples, more than 8 window sizes or more than 1024 ERB points; and the
    case in which swipep itself raises "A value in x_new is outside the interpolation range." (the same message)."""
    x = np.asarray(x)
    if x.ndim != 1 or x.dtype == object or not (np.issubdtype(x.dtype, np.number) or x.dtype == bool):
        raise ValueError("x must be a 1-D array of numbers")
    if np.iscomplexobj(x):
        raise ValueError("x must be real")
    x = np.ascontiguousarray(x, dtype=np.float64)
    if len(x) == 0:
        raise ValueError("x is empty")
    if not np.isfinite(x).all():
        raise ValueError("x must be finite")
    fs, lo, hi = _limits(fs, plim)
    _check_grid(fs, lo, hi)
    swipe_plan(len(x), fs, (lo, hi))          # the time interpolation's range
    return x, fs, (lo, hi)


def _check_time_range(t, tshift):
    """swipep's refusal (interp1d's bounds error) when an instant lies outside a window's shifted frame times."""
    if t[0] < tshift[0] or t[-1] > tshift[-1]:
        raise ValueError("A value in x_new is outside the interpolation range.")


def _kernel_matrices(fs, plim):
    """Per window size (j, k, mu, K): the candidates it scores (swipe.py:107-115), its weights and the kernel matrix whose
    row r is _strength_one's k for pc[j[r]] after both normalisations; the last row is zero (never scored)."""
    key = (fs, plim)
    if key in _KERNELS:
        return _KERNELS[key]
    log2pc, pc, ws, pO, d, f = _check_grid(fs, *plim)
    out = []
    for i in range(len(ws)):
        if i == len(ws) - 1:
            j = np.flatnonzero(d - (i + 1) > -1)
            k = np.flatnonzero(d[j] - (i + 1) < 0)
        elif i == 0:
            j = np.flatnonzero(d - (i + 1) < 1)
            k = np.flatnonzero(d[j] - (i + 1) > 0)
        else:
            j = np.flatnonzero(np.abs(d - (i + 1)) < 1)
            k = np.arange(len(j))
        if len(j) == 0 or not np.array_equal(j, np.arange(j[0], j[0] + len(j))):
            raise ValueError("window %d scores no contiguous candidate range" % int(ws[i]))
        lam = d[j[k]] - (i + 1)
        mu = np.ones(len(j))
        mu[k] = 1 - np.abs(lam)
        pcs = pc[j][:-1]
        K = np.zeros((len(j), len(f)))
        if len(pcs):
            q = f[None, :] / pcs[:, None]
            n = np.fix(f[-1] / pcs - 0.75).astype(np.int64)
            cq = np.cos(2 * np.pi * q)
            kk = np.zeros_like(q)
            for prime in _primes_with_one(int(n.max())):      # one pass per "prime", later lobes overwrite
                rows = (prime <= n + 1)[:, None]
                a = np.abs(q - prime)
                kk = np.where(rows & (a < 0.25), cq, kk)
                kk = np.where(rows & (0.25 < a) & (a < 0.75), cq / 2, kk)
            kk = kk * np.sqrt(1.0 / f)[None, :]
            for r in range(len(pcs)):                         # the norm as _strength_one takes it, row by row
                K[r] = kk[r] / np.linalg.norm(kk[r][kk[r] > 0.0])
        out.append((j, k, mu, K))
    return _remember(_KERNELS, key, out)


def swipe_plan(n, fs, plim):
    """Everything the kernels need that depends on (n, fs, plim) alone, formed with the NumPy expressions of swipe.py
    (host only, no GPU, cached on (n, fs, tuple(plim))): a dict with
        t float64[T], pc, ws, d, fERBs; windows: a list, largest window first, of dicts with
            w, hop, pad (zeros in front), nframes, window (Hann), sumw2, lo int32[nE], xlo, df (the ERB interpolation:
            lower bin, f_e - f[lo], f[lo + 1] - f[lo]), j0, ncand, j, mu, K float64[ncand, nE], tshift float64[nframes];
        ntc float64[npc, 3], nftc, ptab float64[npc, nfmax], nf int32[npc]: the refinement tables of candidate i (rows 0
            and npc - 1 are empty): ptab[i][k] = 2 ** (log2(pc[i - 1]) + (k - 1) / 768) as a scalar power, as swipep does.
    ValueError where check_swipe_arguments would raise for these sizes."""
    n = int(n)
    fs, lo, hi = _limits(fs, plim)
    key = (n, fs, (lo, hi))
    if key in _PLANS:
        return _PLANS[key]
    if n < 1:
        raise ValueError("x is empty")
    log2pc, pc, ws, pO, d, fERBs = _check_grid(fs, lo, hi)
    t = np.arange(0, n / float(fs), 0.001)
    windows = []
    for i, (j, k, mu, K) in enumerate(_kernel_matrices(fs, (lo, hi))):
        w_i = int(ws[i])
        dn = int(round(4 * fs / pO[i]))
        total = w_i // 2 + n + int(dn + w_i / 2)              # length of swipe.py's padded copy
        o = max(0, int(round(w_i - dn)))
        hop = w_i - o
        nframes = (total - o) // hop
        window = np.hanning(w_i)
        f = np.arange(w_i // 2 + 1) * (fs / w_i)
        ti = np.arange(w_i / 2, total - w_i / 2 + 1, hop) / fs
        if len(ti) != nframes or nframes < 2 or not 1 <= hop <= w_i:
            raise ValueError("window %d: %d frames for %d frame times" % (w_i, nframes, len(ti)))
        tshift = np.concatenate(([0.0], ti[:-1]))
        _check_time_range(t, tshift)
        upper = np.clip(np.searchsorted(f, fERBs), 1, len(f) - 1)
        lower = upper - 1
        windows.append(dict(w=w_i, hop=hop, pad=w_i // 2, nframes=int(nframes), window=window,
                            sumw2=float((np.abs(window) ** 2).sum()), lo=lower.astype(np.int32),
                            xlo=fERBs - f[lower], df=f[upper] - f[lower], j0=int(j[0]), ncand=len(j), j=j, mu=mu, K=K,
                            tshift=tshift))
    npc = len(pc)
    fine = [None] * npc
    ntc = np.zeros((npc, 3))
    for i in range(1, npc - 1):
        I = np.arange(i - 1, i + 2)
        tc = 1.0 / pc[I]
        ntc[i] = ((tc / tc[1]) - 1) * 2 * np.pi
        ftc = 1.0 / np.power(2, np.arange(np.log2(pc[I[0]]), np.log2(pc[I[2]]), 0.0013021))
        fine[i] = ((ftc / tc[1]) - 1) * 2 * np.pi
    nf = np.array([0 if v is None else len(v) for v in fine], dtype=np.int32)
    nfmax = int(nf.max())
    if not 1 <= nfmax <= SWIPE_FINE_MAX:
        raise ValueError("a fine grid of %d points, the limit is %d" % (nfmax, SWIPE_FINE_MAX))
    nftc, ptab = np.zeros((npc, nfmax)), np.zeros((npc, nfmax))
    for i in range(1, npc - 1):
        nftc[i, :nf[i]] = fine[i]
        base = np.log2(pc[i - 1])
        for kk in range(nf[i]):
            ptab[i, kk] = 2 ** (base + (int(kk) - 1) / 768)
    plan = dict(n=n, fs=fs, plim=(lo, hi), t=t, pc=pc, ws=ws, d=d, fERBs=fERBs, windows=windows, ntc=ntc, nftc=nftc,
                ptab=ptab, nf=nf, nfmax=nfmax)
    return _remember(_PLANS, key, plan)


def _device_plan(plan, torch, dev):
    """The plan's arrays on the device, kept with the plan."""
    key = (plan["n"], plan["fs"], plan["plim"], str(dev))
    if key in _DEVICE_PLANS:
        return _DEVICE_PLANS[key]
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    on = dict(t=up(plan["t"]), ntc=up(plan["ntc"]), nftc=up(plan["nftc"]), ptab=up(plan["ptab"]), nf=up(plan["nf"]),
              windows=[{k: up(w[k]) for k in ("window", "lo", "xlo", "df", "mu", "K", "tshift")}
                       for w in plan["windows"]])
    return _remember(_DEVICE_PLANS, key, on)


def swipep_device(x, fs, plim, *, device_index=0, return_strengths=False):
    """Pitch track of `x` every 1 ms on the device: float64[T, 3] [time s, pitch Hz, strength], swipe.swipep's layout,
    its time column bit for bit, and its pitch bit for bit wherever the two maxima that decide it (over the candidates,
    then over the candidate's fine grid) are not ties within rounding.  With return_strengths=True also
    S float64[len(pc), T], the combined strengths before the maximum; without it that matrix is never formed.  `x` is
    uploaded once, everything up to the result runs on the context's stream, and only the result comes back.  The same
    bits on every call."""
    x, fs, plim = check_swipe_arguments(x, fs, plim)
    plan = swipe_plan(len(x), fs, plim)
    from .records import _device
    torch, c, dev = _device(device_index)
    on = _device_plan(plan, torch, dev)
    x_d = torch.as_tensor(x, device=dev)
    nE, T, npc = len(plan["fERBs"]), len(plan["t"]), len(plan["pc"])
    wins = []
    for w, w_d in zip(plan["windows"], on["windows"]):
        L = torch.empty((w["nframes"], nE), dtype=torch.float64, device=dev)
        Si = torch.empty((w["ncand"], w["nframes"]), dtype=torch.float64, device=dev)
        c.swipe_loudness(x_d, len(x), w["w"], w["hop"], w["pad"], w["nframes"], w_d["window"], fs, w["sumw2"], w_d["lo"],
                         w_d["xlo"], w_d["df"], nE, L, nE)
        c.swipe_scores(w_d["K"], w["ncand"], nE, L, w["nframes"], nE, nE, Si)
        wins.append((Si, w["j0"], w["ncand"], w["nframes"], w_d["mu"], w_d["tshift"]))
    ps = torch.empty((2, T), dtype=torch.float64, device=dev)
    S = torch.empty((npc, T), dtype=torch.float64, device=dev) if return_strengths else None
    c.swipe_pick(wins, on["t"], T, npc, plan["pc"][0], on["ntc"], on["nftc"], on["ptab"], on["nf"], plan["nfmax"], ps[0],
                 ps[1], S)
    ps_h = ps.cpu().numpy()
    track = np.column_stack((plan["t"], ps_h[0], ps_h[1]))
    return (track, S.cpu().numpy()) if return_strengths else track


def analysis_pitch_track(speechFile, gender, fc=0, *, device_index=0):
    """The pitch track eaQHMAnalysisAndSynthesis(speechFile, gender, fc=fc) would compute with swipe.swipep, from the
    device: prologue.read_signal, prologue.pitch_limits and swipep_device.  Hand it over as pitch_track= (or in
    pitch_tracks=[...] of the batch entry)."""
    from . import prologue
    fs, s = prologue.read_signal(speechFile, fc)
    f0min, f0max = prologue.pitch_limits(gender)
    return swipep_device(s, fs, [f0min, f0max], device_index=device_index)


# ---- the continuous track
def _number(v, name, lo=None):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (name, v)) from None
    if not np.isfinite(v) or (lo is not None and v < lo):
        raise ValueError("%s must be finite%s, got %r" % (name, "" if lo is None else " and >= %g" % lo, v))
    return v


def viterbi_costs(npc, jump_cost=4.0, free_jump=1 / 48, max_jump=0.5):
    """The cost of a step of k candidates between neighbouring instants, float64[W + 1].  The arguments are in octaves
    per step (a candidate is 1/96 octave): jump_cost >= 0 per octave beyond the free part, 0 <= free_jump <= max_jump.
        W = min(npc - 1, 256, max(0, round(96 max_jump))), k0 = round(96 free_jump), cost[k] = jump_cost max(0, k - k0) / 96
    ValueError for anything else, and for npc outside [3, 1024]."""
    npc = _candidates(npc)
    jump_cost = _number(jump_cost, "jump_cost", 0)
    free_jump = _number(free_jump, "free_jump", 0)
    max_jump = _number(max_jump, "max_jump", 0)
    if free_jump > max_jump:
        raise ValueError("free_jump %g exceeds max_jump %g" % (free_jump, max_jump))
    W = min(npc - 1, VITERBI_JUMP_MAX, max(0, int(round(96 * min(max_jump, 1e6)))))
    k0 = int(round(96 * min(free_jump, 1e6)))
    return jump_cost * np.maximum(0, np.arange(W + 1) - k0) / 96


def _candidates(npc):
    if isinstance(npc, bool) or not isinstance(npc, (int, np.integer)):
        raise ValueError("npc must be an integer, got %r" % (npc,))
    if not 3 <= npc <= VITERBI_NPC_MAX:
        raise ValueError("%d pitch candidates: the decode takes 3 to %d" % (npc, VITERBI_NPC_MAX))
    return int(npc)


def _check_cost(cost, npc):
    cost = np.asarray(cost)
    if cost.ndim != 1 or cost.dtype == object or not np.issubdtype(cost.dtype, np.number) or np.iscomplexobj(cost):
        raise ValueError("cost must be a 1-D array of real numbers")
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    if not 1 <= len(cost) <= min(npc - 1, VITERBI_JUMP_MAX) + 1:
        raise ValueError("cost has %d entries: 1 to min(npc - 1, %d) + 1 = %d are possible"
                         % (len(cost), VITERBI_JUMP_MAX, min(npc - 1, VITERBI_JUMP_MAX) + 1))
    if not (np.isfinite(cost).all() and (cost >= 0).all()):
        raise ValueError("cost must be finite and >= 0")
    return cost


def _check_unvoiced(unvoiced, voicing_cost):
    """None, or (uv, vcost) as floats."""
    if unvoiced is None:
        return None
    return _number(unvoiced, "unvoiced"), _number(voicing_cost, "voicing_cost", 0)


def _device_index(device_index):
    if isinstance(device_index, bool) or not isinstance(device_index, (int, np.integer)) or device_index < 0:
        raise ValueError("device_index must be a non-negative integer, got %r" % (device_index,))
    return int(device_index)


def _decode(torch, c, dev, S_d, npc, T, cost, unvoiced):
    """Forward and backtrack over the device matrix S_d: (q int32[T], last float64[npc + 1]) on the device."""
    ntiles = -(-T // VITERBI_TILE)
    cost_d = torch.as_tensor(cost, device=dev)
    bp = torch.empty((T, npc + 1), dtype=torch.int16, device=dev)
    tilemap = torch.empty((ntiles, npc + 1), dtype=torch.int16, device=dev)
    last = torch.empty(npc + 1, dtype=torch.float64, device=dev)
    q = torch.empty(T, dtype=torch.int32, device=dev)
    c.viterbi_forward(S_d, npc, T, cost_d, len(cost) - 1, unvoiced, bp, tilemap, last)
    c.viterbi_backtrack(bp, tilemap, last, npc, T, q)
    return q, last


def viterbi_track(S, cost, *, unvoiced=None, voicing_cost=1.0, device_index=0):
    """The best path through S float64[npc, T] (any host matrix: SWIPE' strengths, or those plus a term of the caller's)
    under the step costs `cost` (viterbi_costs, or any finite table >= 0 of at most min(npc - 1, 256) + 1 entries): the
    path maximises the sum of S[q[t], t] minus cost[|q[t] - q[t-1]|], steps beyond len(cost) - 1 candidates excluded.
    With `unvoiced` = the score of an unvoiced instant, state npc is "unvoiced", entered and left at voicing_cost.
    Returns (q int32[T], last float64[npc + 1]): the path and the scores of the last instant, last[npc] = -inf without
    the unvoiced state.  The recurrence and its tie rules are DESIGN.md §13.1; the same bits on every call."""
    S = np.asarray(S)
    if S.ndim != 2 or S.dtype == object or not np.issubdtype(S.dtype, np.number) or np.iscomplexobj(S):
        raise ValueError("S must be a 2-D array of real numbers [candidates, instants]")
    npc = _candidates(S.shape[0])
    T = S.shape[1]
    if not 1 <= T < 2 ** 31:
        raise ValueError("S has %d instants, 1 to 2^31 - 1 are possible" % T)
    S = np.ascontiguousarray(S, dtype=np.float64)
    if not np.isfinite(S).all():
        raise ValueError("S must be finite")
    cost = _check_cost(cost, npc)
    unvoiced = _check_unvoiced(unvoiced, voicing_cost)
    device_index = _device_index(device_index)
    from .records import _device
    torch, c, dev = _device(device_index)
    q, last = _decode(torch, c, dev, torch.as_tensor(S, device=dev), npc, T, cost, unvoiced)
    return q.cpu().numpy(), last.cpu().numpy()


def fill_unvoiced(p, voiced, default):
    """The pitch column of a track with unvoiced instants: an unvoiced instant carries the pitch of the nearest EARLIER
    voiced instant, else of the next later one; without any voiced instant `default` everywhere."""
    p = np.array(p, dtype=np.float64)
    voiced = np.asarray(voiced, dtype=bool)
    at = np.flatnonzero(voiced)
    if len(at) == 0:
        p[:] = default
        return p
    i = np.searchsorted(at, np.arange(len(p)), side="right") - 1      # the last voiced instant at or before each
    return p[at[np.maximum(i, 0)]]


def _strengths_on_device(x, plan, torch, c, dev):
    """swipep_device's three stages with the strength matrix kept: S float64[npc, T] on the device."""
    on = _device_plan(plan, torch, dev)
    x_d = torch.as_tensor(x, device=dev)
    fs, nE, T, npc = plan["fs"], len(plan["fERBs"]), len(plan["t"]), len(plan["pc"])
    wins = []
    for w, w_d in zip(plan["windows"], on["windows"]):
        L = torch.empty((w["nframes"], nE), dtype=torch.float64, device=dev)
        Si = torch.empty((w["ncand"], w["nframes"]), dtype=torch.float64, device=dev)
        c.swipe_loudness(x_d, len(x), w["w"], w["hop"], w["pad"], w["nframes"], w_d["window"], fs, w["sumw2"], w_d["lo"],
                         w_d["xlo"], w_d["df"], nE, L, nE)
        c.swipe_scores(w_d["K"], w["ncand"], nE, L, w["nframes"], nE, nE, Si)
        wins.append((Si, w["j0"], w["ncand"], w["nframes"], w_d["mu"], w_d["tshift"]))
    ps = torch.empty((2, T), dtype=torch.float64, device=dev)
    S = torch.empty((npc, T), dtype=torch.float64, device=dev)
    c.swipe_pick(wins, on["t"], T, npc, plan["pc"][0], on["ntc"], on["nftc"], on["ptab"], on["nf"], plan["nfmax"], ps[0],
                 ps[1], S)
    return on, S


def swipep_viterbi(x, fs, plim, *, jump_cost=4.0, free_jump=1 / 48, max_jump=0.5, unvoiced=None, voicing_cost=1.0,
                   device_index=0, return_path=False):
    """swipep_device's track with the pitch taken along the best continuous path through the strengths instead of at
    each instant's own maximum: float64[T, 3] [time s, pitch Hz, strength], the time column bit for
    bit swipep's.  A step of k candidates costs viterbi_costs(npc, jump_cost, free_jump, max_jump)[k].  With `unvoiced`
    (the score of an unvoiced instant, 0.2 is a usual value) the path decides voicing too, at voicing_cost a change; an
    unvoiced instant carries the pitch of the nearest earlier voiced instant (else of the next later one) and strength
    0, and a track without a voiced instant carries pc[0].  On the path the pitch and strength are swipep's refinement
    of the path's candidate; on an edge candidate they are that candidate's pitch and strength (swipep maps both edges
    to pc[0]).  The strengths stay on the device; only the result comes back.  With return_path=True:
    (track, q int32[T] with len(pc) for unvoiced, voiced bool[T])."""
    x, fs, plim = check_swipe_arguments(x, fs, plim)
    plan = swipe_plan(len(x), fs, plim)
    npc, T = len(plan["pc"]), len(plan["t"])
    if npc > VITERBI_NPC_MAX:
        raise ValueError("plim [%g, %g] gives %d pitch candidates, the limit of the decode is %d"
                         % (plim[0], plim[1], npc, VITERBI_NPC_MAX))
    cost = viterbi_costs(npc, jump_cost, free_jump, max_jump)
    unvoiced = _check_unvoiced(unvoiced, voicing_cost)
    device_index = _device_index(device_index)
    from .records import _device
    torch, c, dev = _device(device_index)
    on, S = _strengths_on_device(x, plan, torch, c, dev)
    q, _ = _decode(torch, c, dev, S, npc, T, cost, unvoiced)
    if "pc" not in on:
        on["pc"] = torch.as_tensor(np.ascontiguousarray(plan["pc"]), device=dev)
    ps = torch.empty((2, T), dtype=torch.float64, device=dev)
    c.viterbi_refine(S, q, npc, T, on["pc"], on["ntc"], on["nftc"], on["ptab"], on["nf"], plan["nfmax"], ps[0], ps[1])
    ps_h, q_h = ps.cpu().numpy(), q.cpu().numpy()
    voiced = q_h < npc
    track = np.column_stack((plan["t"], fill_unvoiced(ps_h[0], voiced, plan["pc"][0]), ps_h[1]))
    return (track, q_h, voiced) if return_path else track


def analysis_pitch_track_viterbi(speechFile, gender, fc=0, *, device_index=0, **options):
    """analysis_pitch_track with swipep_viterbi in place of swipep_device; `options` are swipep_viterbi's (jump_cost,
    free_jump, max_jump, unvoiced, voicing_cost).  Hand the result over as pitch_track= (or in pitch_tracks=[...])."""
    if "return_path" in options:
        raise ValueError("analysis_pitch_track_viterbi returns the track alone: no return_path")
    from . import prologue
    fs, s = prologue.read_signal(speechFile, fc)
    f0min, f0max = prologue.pitch_limits(gender)
    return swipep_viterbi(s, fs, [f0min, f0max], device_index=device_index, **options)
