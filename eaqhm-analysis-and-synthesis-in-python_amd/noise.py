"""The stochastic component: the residual s - s_recon as an LPC envelope and a gain per 5 ms frame,
resynthesised as filtered white noise; its formant scale and warp (§10.1), its pitch-synchronous modulation (§10.2)
and its way to and from cepstral rows (§10.4).  The work runs in libeaqhm_hip.so (eaqhm_noise_analyse,
eaqhm_noise_synth, eaqhm_noise_warp, eaqhm_noise_envelope, eaqhm_noise_modulation, eaqhm_noise_cepstrum,
eaqhm_noise_from_cepstrum); there is no CPU path.

    eaQHMNoiseAnalysis(s, s_recon, fs, order=None, hop=None, *, device_index=0) -> dict(sigma, refl, hop, order, fs, length)
    eaQHMNoiseSynthesis(noise, tau, L_out, seed=0, fundamental=None, *, device_index=0) -> float64[L_out]
    noise_time_map(hop, L_out, rho) / noise_time_map_contour(hop, tm, step) -> float64[Nq]
    eaQHMNoiseWarp(noise, formant_scale=1.0, *, formant_warp=None, device_index=0) -> dict(sigma, refl, hop, order, fs, length)
    noise_envelope(noise, fs, freqs, formant_scale=1.0, *, formant_warp=None, device_index=0) -> float64[Nf, len(freqs)]
    noise_formant_contour(noise, DetComponents, formant_scale) -> float64[Nf]
    noise_formant_warp(noise, DetComponents, formant_warp) -> (f_in[B], f_out[Nf, B])
    noise_cepstrum(noise, order=63, *, device_index=0) -> float64[Nf, order + 1]
    noise_from_cepstrum(ceps, hop, fs, *, order=None, length=None, mod=None, mod_harmonics=None, cep_warp=0.0,
                        device_index=0) -> dict(sigma, refl, hop, order, fs, length)
    noise_alignment_index(idx, detA, noiseA, detB, noiseB) -> float64[NfA]
    eaQHMNoiseModulation(s, s_recon, noise, DetComponents, harmonics=2, f0=None, *, device_index=0) -> noise + mod
    noise_fundamental(DetComponents, fs, tau, time_map=None, time_scale=1.0, pitch_scale=1.0, f0=None) -> (theta, nu)

Argument checks without device work: check_noise_model(noise), check_noise_analysis_arguments(s, s_recon, fs,
order=None, hop=None), check_noise_synthesis_arguments(noise, tau, L_out, seed=0), check_noise_formant(noise_formant,
noise, preserve_envelope), check_noise_warp_arguments(noise, formant_scale), check_noise_warp_map_arguments(noise,
formant_warp, formant_scale=1.0), check_noise_envelope_arguments(noise, fs, freqs, formant_scale),
check_noise_cepstrum_arguments(noise, order=63), check_noise_from_cepstrum_arguments(ceps, hop, fs, order=None,
length=None, mod=None, mod_harmonics=None), check_noise_fundamental(nz, fundamental, Nq),
check_noise_modulation(noise_modulation, nz), check_noise_modulation_arguments(s, s_recon, noise, DetComponents,
harmonics=2, f0=None).  Constants: NOISE_MAX_HOP, NOISE_MAX_ORDER, NOISE_MOD_MAX, NOISE_CEPSTRUM_EXP_MAX,
NOISE_CEPSTRUM_LEVEL_MAX.
"""
import numpy as np

from .args import (_contour, _freq_grid, _in_range, _integer, _is_contour, _numeric_1d, _sample_rate, _scale, _seed,
                   _warp_excludes_scale, _warp_rows)
from .records import (_check_records, _device, _frac, _records_phase, check_phase_arguments, fundamental_advance,
                      unpack_model)
from .cepstrum import _cepstrum_order, _cepstrum_rows, _on_axis, check_cepstrum_warp

NOISE_MAX_HOP = 1024     # the analysis kernel keeps one 4-hop frame per wave in LDS
NOISE_MAX_ORDER = 63     # lane l of a wave owns lag l
NOISE_MOD_MAX = 8        # harmonics of the pitch-synchronous envelope of the noise at most


# ---- the stochastic component
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
