"""Resynthesis from an analysed eaQHM model, with time, pitch and formant scaling (not in the reference), and the
one import point of the whole model layer.

    eaQHMSynthesis(DetComponents, fs, length, time_scale=1.0, pitch_scale=1.0, preserve_envelope=True,
                   formant_scale=1.0, *, phase="independent", f0=None, noise=None, noise_seed=0, noise_formant=False,
                   noise_modulation=False, formant_warp=None, envelope=None, cep_warp=0.0, device_index=0)
        -> float64[L_out]
    model_envelope(DetComponents, fs, freqs, formant_scale=1.0, formant_warp=None, *, device_index=0)
        -> float64[No_ti, len(freqs)]
    check_arguments(model, fs, length, time_scale, pitch_scale) -> (rho, beta, fs, length)
    check_contour_arguments(model, fs, length, time_scale, pitch_scale) -> (rho, beta, fs, length), rho, beta float64[No_ti]
    check_envelope_arguments(model, fs, freqs, formant_scale)

At time_scale = pitch_scale = 1 the result is the analysis's own s_recon; the definition for other settings is in
DESIGN.md ("Resynthesis from the model", §9).  Either scale may also be a contour, one value per analysis instant
(§9.1); a formant scale or a formant warp moves the spectral envelope on its own (§9.2, §9.4); phase="shape" keeps the
waveform shape of a pitch period at every scale (§11).  The work runs in libeaqhm_hip.so (eaqhm_spline_solve,
eaqhm_modify_prep, eaqhm_modify_synth, eaqhm_modify_amp_cepstrum, eaqhm_model_envelope); there is no CPU path.

The synthesis sits on top of five modules, each of which imports only from the ones before it:

    args      the argument rules that take no model (scales, contours, curves, integers, warp breakpoints)
    records   unpack_model, the device records, and the fundamental, phase and time map read off them
    cepstrum  the discrete-cepstrum envelope, the model built from parameters, the warped axis
    align     banded DTW over cepstral rows
    noise     the stochastic component: LPC model, warp, cepstral rows, pitch-synchronous modulation

Every name of theirs is imported here by name, so `from eaqhm_amd.model import X` reaches all of them; cli resolves the
public functions through this module at call time.
"""
import numpy as np

from .args import (FORMANT_WARP_MAX, SCALE_RANGE, _contour, _freq_grid, _in_range, _integer, _is_contour,  # noqa: F401
                   _numeric_1d, _sample_rate, _scale, _seed, _warp_excludes_scale, _warp_rows, check_curve)
from .records import (PHASE_MODES, _cells, _check_records, _device, _device_records, _frac,  # noqa: F401
                      _model_instants, _records_f0, _records_phase, check_formant_scale,
                      check_formant_warp, check_phase_arguments, contour_time_map, formant_warp_vtln,
                      fundamental_advance, model_f0, model_phase, scale_contour, unpack_model)
from .cepstrum import (BUILD_MAX_HARMONICS, BUILD_PHASES, CEPSTRUM_LAMBDA_RANGE, CEPSTRUM_MAX_ORDER,  # noqa: F401
                       CEPSTRUM_WARP_MAX, CEPSTRUM_WARP_SCALES, _cepstrum_lambda, _cepstrum_order,
                       _cepstrum_rows, _held, _on_axis, allpass_warp, cepstrum_envelope, cepstrum_phase,
                       cepstrum_rewarp, cepstrum_warp, check_cepstrum_rewarp_arguments,
                       check_cepstrum_warp, check_envelope_cepstrum, check_model_build_arguments,
                       check_model_cepstrum_arguments, fundamental_phase, harmonic_counts, model_cepstrum,
                       model_from_parameters, model_parameters, rewarp_matrix)
from .align import (_band_radius, _cost_weight, _fits_device, _path, _run_dtw, alignment_index,  # noqa: F401
                    alignment_time_scale, band_centres, band_min_radius, check_dtw_arguments,
                    check_model_align_arguments, dense_to_band, dtw, model_align, warp_rows)
from .noise import (NOISE_CEPSTRUM_EXP_MAX, NOISE_CEPSTRUM_LEVEL_MAX, NOISE_MAX_HOP, NOISE_MAX_ORDER,  # noqa: F401
                    NOISE_MOD_MAX, _device_mod, _device_noise_warp, _device_noise_warp_map, _frame_alpha,
                    _frame_rows, _fundamental_at, _mod_harmonics, _noise_shape, _phase_at, _scalar_path,
                    _signal_pair, _tau, _warp_normalised, check_noise_analysis_arguments,
                    check_noise_cepstrum_arguments, check_noise_envelope_arguments, check_noise_formant,
                    check_noise_from_cepstrum_arguments, check_noise_fundamental, check_noise_model,
                    check_noise_modulation, check_noise_modulation_arguments,
                    check_noise_synthesis_arguments, check_noise_warp_arguments,
                    check_noise_warp_map_arguments, eaQHMNoiseAnalysis, eaQHMNoiseModulation,
                    eaQHMNoiseSynthesis, eaQHMNoiseWarp, noise_alignment_index, noise_cepstrum,
                    noise_envelope, noise_formant_contour, noise_formant_warp, noise_from_cepstrum,
                    noise_fundamental, noise_time_map, noise_time_map_contour)


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


def check_contour_arguments(model, fs, length, time_scale, pitch_scale):
    """check_arguments for contours (no device work): either scale may be a number (broadcast) or a 1-D array of one
    value per analysis instant.  Returns (rho, beta, fs, length) with rho, beta float64[No_ti]."""
    n = len(model["ti"])
    rho = _contour(time_scale, "time_scale", n)
    beta = _contour(pitch_scale, "pitch_scale", n)
    _, _, fs, length = check_arguments(model, fs, length, 1.0, 1.0)
    return rho, beta, fs, length


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
