"""Headless replacement for the reference's GUI harness main.py:44-72 (no Tk dialog, no plots):

    python eaqhm_amd.py <file.wav> [--gender female] [--max-adpt 10] ...

prints the per-adaptation SRER lines in the reference's format (functions.py:391-392, :415-416) and writes
`<name>_reconstructed.wav` as float32 next to the input (main.py:72).  With --time-scale / --pitch-scale it also
resynthesises the analysed model (model.eaQHMSynthesis) into `<name>_modified.wav` (float32).  --time-scale-curve /
--pitch-scale-curve FILE take a breakpoint curve instead (two whitespace-separated columns, seconds and value; lines
starting with # are comments), turned into a per-instant contour with model.scale_contour.  --formant-scale A /
--formant-scale-curve FILE move the spectral envelope by A; they need the envelope, so either one with
--no-envelope is an error.  --formant-warp-curve FILE (two columns, Hz in the model and Hz in the output) and
--formant-vtln ALPHA (with --formant-knee K, default 0.875) move it along a piecewise-linear map instead (DESIGN.md
§9.4); the four formant flags exclude each other.  --phase shape keeps the waveform shape under those scales.  --noise (with --noise-seed N) models the residual input - reconstruction
(model.eaQHMNoiseAnalysis) and adds its resynthesis to `<name>_modified.wav`; without any scale flag it
writes `<name>_resynthesis.wav`: model + noise at unit scales.  --noise-formant (with --noise and a formant scale flag) lets the
noise's envelope follow the formant scale or warp (eaQHMSynthesis(noise_formant=True)).  --noise-modulation [M]
(with --noise; M harmonics, default 2) modulates the noise pitch-synchronously (model.eaQHMNoiseModulation).
--cepstral-envelope [P] (with --cepstral-lambda L, default 5e-4) reads the amplitudes of `<name>_modified.wav` off the model's
own discrete-cepstrum envelope of order P (model.model_cepstrum; P defaults to min(63, 2 + round(fs / 1000)));
it goes with any scale flag and not with --no-envelope.  --envelope-from OTHER.wav analyses OTHER with the same options, fits
both cepstra (order and lambda of --cepstral-envelope / --cepstral-lambda, or their defaults), aligns the two in time
(model.model_align) and reads the amplitudes of `<name>_modified.wav` off OTHER's envelope at the aligned
instants; --timing-from OTHER.wav gives the output OTHER's local tempo instead of a --time-scale
(model.alignment_time_scale).  --align-band SECONDS (2.0) is the half-width of the alignment band, raised to the least
that admits a path.  --from-parameters [P] reduces the analysed model to f0, voicing and a cepstrum of order P
(model.model_parameters; lambda from --cepstral-lambda), rebuilds a harmonic model from those arrays alone with the
envelope's minimum-phase response as its phases (model.model_from_parameters) and writes its synthesis, under
whatever scale, formant, phase and noise flags are given, as `<name>_vocoded.wav`; not with --no-envelope.
--noise-cepstrum [Q] (with --noise; Q in 1..63, default 63) passes the noise model through its cepstral rows and back
(model.noise_cepstrum, model.noise_from_cepstrum).  --noise-from OTHER.wav (with --noise) analyses OTHER
with the same options (once, if --envelope-from / --timing-from name the same file), models its residual, aligns the two
files as --envelope-from does and puts OTHER's noise at this file's timing (model.noise_alignment_index) in place of its
own; it implies --noise-cepstrum and does not go with --noise-modulation.
--conversion-train TARGET.wav --conversion-save MAP.npz (with --conversion-components M, default 8) analyses TARGET with the
same options, fits both cepstra (order and lambda of --cepstral-envelope / --cepstral-lambda, or their defaults), aligns the
two, pairs the aligned rows (convert.conversion_pairs) and learns the map from this file's rows to TARGET's as a joint
Gaussian mixture (convert.conversion_train); MAP.npz holds the map, the order, lambda, fs and both speakers'
ln f0 statistics.  --conversion MAP.npz fits this file's cepstrum at the map's order and lambda, converts it
(convert.conversion_apply) and reads the amplitudes of `<name>_modified.wav` off the result; unless a pitch flag is given the
pitch follows the target speaker's statistics (convert.pitch_conversion_contour).  A different explicit --cepstral-envelope P
or a different fs is an error; not with --envelope-from, --no-envelope or --conversion-train.
--conversion-span L (with --conversion-train; L in 1..8, 2 is the usual choice) learns a dynamic map instead: both cepstra are
extended with their delta features over a window of L instants a side before the pairing (convert.conversion_pairs(span=)),
the mixture is over the extended rows, and MAP.npz carries the span.  --conversion MAP.npz with such a map converts this
file to the most likely trajectory under the static and the delta statistics (convert.conversion_trajectory, DESIGN.md
§12.1) in place of the row-by-row rule, so that the converted envelope does not jump where the posterior changes component.
--conversion-init axis|kmeans (with --conversion-train) chooses where EM starts: `axis`, the default, cuts the rows into
equal runs along their principal axis; `kmeans` starts from a k-means codebook of M centres grown by splitting
(convert.kmeans).
--conversion-gv [S] (with --conversion-train and --conversion-span) also stores the target's global-variance statistics in
MAP.npz (convert.gv_statistics of TARGET's cepstrum): the variance of each coefficient over the utterance, with a stated
relative spread S (0.25 when left out: one utterance has no spread of its own).  --conversion MAP.npz with such a map adds
the global-variance term to the trajectory, which gives the converted coefficients the target's variance
back; --conversion-no-gv switches it off, --conversion-gv-iters K (30) and --conversion-gv-weight G (1) set the number of
sweeps and the weight of the term.
--conversion-em-iters K (with --conversion and a dynamic map; K in 0..100) revises the mixture's component posteriors in
the light of the trajectory and solves it again, K times, before the global-variance term
(convert.conversion_trajectory_em); without the flag the conversion is convert.conversion_trajectory.
--conversion-nonparallel [R] (with --conversion-train; R in 1..50, default 8) is for a TARGET.wav that is NOT the same
sentence: both cepstra are fitted as above, nothing is aligned, and the map is learned by up to R rounds of nearest-row
pairing and training (nonparallel.conversion_train_nonparallel, INCA).  With --conversion-span (and
--conversion-gv) the dynamic map is then trained from the last pairs.  MAP.npz has the same fields.
--cepstral-warp A|mel|bark (with --cepstral-envelope, --from-parameters, --envelope-from, --timing-from, --conversion-train
or --conversion) puts every cepstrum of the model on the all-pass warped frequency axis of DESIGN.md §9.8: a number in
[-0.9, 0.9], or the coefficient model.cepstrum_warp gives for the file's sampling rate.  --conversion-train stores it in
MAP.npz, and --conversion MAP.npz fits at the map's axis (a map without the entry lies on the linear axis); a different
explicit --cepstral-warp is an error.  The noise flags keep their linear rows.
--pitch-device takes the pitch track of the analysis, and of the analyses of --envelope-from, --timing-from, --noise-from
and --conversion-train, from the device (pitch.analysis_pitch_track) in place of the host's swipe.swipep.
--pitch-viterbi takes it from pitch.analysis_pitch_track_viterbi instead: the device's strengths, and
the pitch along the best continuous path through them rather than at each instant's own maximum; it implies the device
estimator.  --pitch-jump-cost C (4) is the cost of a jump per octave, and --pitch-unvoiced U (0.2 is a usual value) adds an
unvoiced state with the score U per instant, so that the path decides voicing too; both need --pitch-viterbi.
--formants-out FILE measures the formants of the input (formant.signal_allpole, formant_candidates, formant_tracks,
DESIGN.md §14) and writes one line per 5 ms frame: seconds, F1..FN, B1..BN in Hz, nan where a formant is absent;
--formant-count N (1 to 4, default 3) sets N.  --formant-warp-from OTHER.wav measures both files' formants and moves this
file's spectral envelope along the piecewise-linear map from its own median formants to OTHER's
(formant.formant_warp_from_tracks); it writes `<name>_modified.wav` and excludes the other four formant flags.
--protect-transients (with --time-scale, --time-scale-curve or --timing-from) finds the input's transient onsets on the
device (transient.onset_strength, transient.onsets) and replaces the time scale by the contour that plays
them at their own duration and stretches the rest a little more, to the same total length
(transient.protect_time_scale); --phase shape goes well with it.  --transient-delta D (0.5) sets the detector's threshold.
--onsets-out FILE writes the onsets, one line `seconds strength` each; it works with or without --protect-transients."""
import argparse

import numpy as np
from scipy.io import wavfile

from .functions import eaQHMAnalysisAndSynthesis


def cepstral_warp_argument(text):
    """--cepstral-warp: 'mel', 'bark' or a number in [-0.9, 0.9]."""
    from .model import CEPSTRUM_WARP_MAX, CEPSTRUM_WARP_SCALES
    if text in CEPSTRUM_WARP_SCALES:
        return text
    try:
        a = float(text)
    except ValueError:
        a = float("nan")
    if not abs(a) <= CEPSTRUM_WARP_MAX:
        raise argparse.ArgumentTypeError("%r is not mel, bark or a number in [-%g, %g]"
                                         % (text, CEPSTRUM_WARP_MAX, CEPSTRUM_WARP_MAX))
    return a


def analyse(path, gender, analysis_options):
    """eaQHMAnalysisAndSynthesis(path, gender, **analysis_options); with the entry pitch_device (--pitch-device) the pitch
    track is pitch.analysis_pitch_track's, with the entry pitch_viterbi (--pitch-viterbi: a dict of
    analysis_pitch_track_viterbi's options, possibly empty) that function's."""
    options = dict(analysis_options)
    viterbi = options.pop("pitch_viterbi", None)
    if viterbi is not None:
        from .pitch import analysis_pitch_track_viterbi
        options.pop("pitch_device", None)
        options["pitch_track"] = analysis_pitch_track_viterbi(path, gender, options.get("fc", 0), **viterbi)
    elif options.pop("pitch_device", False):
        from .pitch import analysis_pitch_track
        options["pitch_track"] = analysis_pitch_track(path, gender, options.get("fc", 0))
    return eaQHMAnalysisAndSynthesis(path, gender, **options)


def parser():
    ap = argparse.ArgumentParser(prog="eaqhm_amd", description="eaQHM analysis/resynthesis on MI355X")
    ap.add_argument("wav")
    ap.add_argument("--gender", default="other", help="male | female | child | other | fmin,fmax")
    ap.add_argument("--step", type=int, default=15)
    ap.add_argument("--max-adpt", type=int, default=10)
    ap.add_argument("--pitch-periods", type=int, default=3)
    ap.add_argument("--analysis-window", type=int, default=32)
    ap.add_argument("--voiced-only", action="store_true", help="fullWaveform=False")
    ap.add_argument("--fc", type=int, default=0)
    ap.add_argument("--partials", type=int, default=0)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--pitch-device", action="store_true",
                    help="SWIPE' on the device (pitch.analysis_pitch_track) for every analysis of this run")
    ap.add_argument("--pitch-viterbi", action="store_true",
                    help="the pitch along the best continuous path through the device's SWIPE' strengths "
                         "(pitch.analysis_pitch_track_viterbi) for every analysis of this run; implies --pitch-device")
    ap.add_argument("--pitch-jump-cost", type=float, default=None, metavar="C",
                    help="with --pitch-viterbi: the cost of a pitch jump per octave, >= 0 (4)")
    ap.add_argument("--pitch-unvoiced", type=float, default=None, metavar="U",
                    help="with --pitch-viterbi: add an unvoiced state with the score U per instant (0.2 is a usual value)")
    ap.add_argument("--track-budget-mb", type=float, default=0.0,
                    help="long files: device memory for the dense tracks (streamed in time blocks, same results); 0 = automatic: "
                         "resident while they fit comfortably, streamed otherwise")
    ts = ap.add_mutually_exclusive_group()
    ts.add_argument("--time-scale", type=float, default=None, help="also write <name>_modified.wav: durations x R")
    ts.add_argument("--time-scale-curve", default=None, metavar="FILE",
                    help="like --time-scale, with a curve: lines 'seconds value' (# comments)")
    ts.add_argument("--timing-from", default=None, metavar="OTHER.wav",
                    help="also write <name>_modified.wav: the local tempo of OTHER.wav, aligned in time to this file")
    ps = ap.add_mutually_exclusive_group()
    ps.add_argument("--pitch-scale", type=float, default=None, help="also write <name>_modified.wav: pitch x B")
    ps.add_argument("--pitch-scale-curve", default=None, metavar="FILE",
                    help="like --pitch-scale, with a curve: lines 'seconds value' (# comments)")
    fs_ = ap.add_mutually_exclusive_group()
    fs_.add_argument("--formant-scale", type=float, default=None,
                     help="also write <name>_modified.wav: spectral envelope (formants) x A")
    fs_.add_argument("--formant-scale-curve", default=None, metavar="FILE",
                     help="like --formant-scale, with a curve: lines 'seconds value' (# comments)")
    fs_.add_argument("--formant-warp-curve", default=None, metavar="FILE",
                     help="also write <name>_modified.wav: spectral envelope moved along a piecewise-linear map: lines "
                          "'Hz_in Hz_out' (# comments), 1 to 16 of them, both columns increasing")
    fs_.add_argument("--formant-vtln", type=float, default=None, metavar="ALPHA",
                     help="like --formant-warp-curve, with the VTLN map: slope ALPHA up to the knee, then straight to "
                          "(fs/2, fs/2)")
    fs_.add_argument("--formant-warp-from", default=None, metavar="OTHER.wav",
                     help="like --formant-warp-curve, with the map from this file's median formants to OTHER.wav's "
                          "(formant.formant_warp_from_tracks)")
    ap.add_argument("--formants-out", default=None, metavar="FILE",
                    help="write the formant tracks of the input: lines 'seconds F1..FN B1..BN' (Hz, nan: absent)")
    ap.add_argument("--formant-count", type=int, default=None, metavar="N",
                    help="with --formants-out / --formant-warp-from: the number of formants, 1 to 4 (3)")
    ap.add_argument("--formant-knee", type=float, default=None, metavar="K",
                    help="with --formant-vtln: the knee as a fraction of fs/2 (0.875)")
    ap.add_argument("--protect-transients", action="store_true",
                    help="with --time-scale, --time-scale-curve or --timing-from: bursts and sharp attacks keep their own "
                         "duration, the rest is stretched a little more (transient.protect_time_scale)")
    ap.add_argument("--transient-delta", type=float, default=None, metavar="D",
                    help="with --protect-transients / --onsets-out: the onset detector's threshold, >= 0 (0.5)")
    ap.add_argument("--onsets-out", default=None, metavar="FILE",
                    help="write the transient onsets of the input: lines 'seconds strength'")
    ap.add_argument("--no-envelope", action="store_true",
                    help="with --pitch-scale: partials keep their amplitudes instead of the spectral envelope's")
    ap.add_argument("--phase", choices=("independent", "shape"), default="independent",
                    help="with a scale flag: 'shape' keeps the harmonics' phases relative to the fundamental (the "
                         "waveform shape of a pitch period) at every scale; 'independent' scales each partial's own")
    ap.add_argument("--noise", action="store_true",
                    help="model the residual as filtered noise and add it to <name>_modified.wav; without a scale flag "
                         "write <name>_resynthesis.wav (model + noise)")
    ap.add_argument("--noise-seed", type=int, default=None, metavar="N", help="with --noise: seed of the excitation (0)")
    ap.add_argument("--noise-formant", action="store_true",
                    help="with --noise and a formant flag (--formant-scale, --formant-scale-curve, --formant-warp-curve, "
                         "--formant-vtln): the noise's spectral envelope follows it")
    ap.add_argument("--noise-modulation", type=int, nargs="?", const=2, default=None, metavar="M",
                    help="with --noise: modulate the noise pitch-synchronously, M harmonics of the envelope (2)")
    ap.add_argument("--noise-cepstrum", type=int, nargs="?", const=63, default=None, metavar="Q",
                    help="with --noise: the noise model goes through its cepstral rows of order Q (1 to 63; 63) and back")
    ap.add_argument("--noise-from", default=None, metavar="OTHER.wav",
                    help="with --noise: the noise of OTHER.wav's residual, aligned in time to this file, in place of this "
                         "file's own (implies --noise-cepstrum; not with --noise-modulation)")
    ap.add_argument("--cepstral-envelope", type=int, nargs="?", const=0, default=None, metavar="P",
                    help="also write <name>_modified.wav: amplitudes read off the model's discrete-cepstrum envelope of "
                         "order P (1 to 63; default min(63, 2 + round(fs / 1000)))")
    ap.add_argument("--cepstral-lambda", type=float, default=None, metavar="L",
                    help="with --cepstral-envelope: the regularisation weight, in [1e-6, 1] (5e-4)")
    ap.add_argument("--cepstral-warp", type=cepstral_warp_argument, default=None, metavar="A|mel|bark",
                    help="with --cepstral-envelope, --from-parameters, --envelope-from, --timing-from or a conversion "
                         "flag: the cepstra lie on the all-pass warped frequency axis with the coefficient A in [-0.9, 0.9], "
                         "or with the one that follows the mel or the Bark scale at the file's sampling rate")
    ap.add_argument("--envelope-from", default=None, metavar="OTHER.wav",
                    help="also write <name>_modified.wav: amplitudes read off the cepstral envelope of OTHER.wav, aligned "
                         "in time to this file (order and lambda: --cepstral-envelope, --cepstral-lambda)")
    ap.add_argument("--from-parameters", type=int, nargs="?", const=0, default=None, metavar="P",
                    help="also write <name>_vocoded.wav: the model rebuilt from its f0, voicing and cepstrum of order P "
                         "(1 to 63; default min(63, 2 + round(fs / 1000))), with minimum-phase harmonics")
    ap.add_argument("--align-band", type=float, default=None, metavar="SECONDS",
                    help="with --envelope-from / --timing-from / --noise-from: half-width of the alignment band (2.0)")
    ap.add_argument("--conversion-train", default=None, metavar="TARGET.wav",
                    help="learn the spectral conversion from this file (source) to TARGET.wav, the same sentence by "
                         "another speaker; needs --conversion-save")
    ap.add_argument("--conversion-save", default=None, metavar="MAP.npz",
                    help="with --conversion-train: where the learned map is written")
    ap.add_argument("--conversion-components", type=int, default=None, metavar="M",
                    help="with --conversion-train: components of the Gaussian mixture, 1 to 64 (8)")
    ap.add_argument("--conversion-span", type=int, default=None, metavar="L",
                    help="with --conversion-train: learn a dynamic map on rows extended with their delta features over L "
                         "instants a side, 1 to 8; --conversion then converts to the most likely trajectory")
    ap.add_argument("--conversion-init", choices=("axis", "kmeans"), default=None,
                    help="with --conversion-train: where EM starts, equal runs along the principal axis (axis, the "
                         "default) or a k-means codebook (kmeans)")
    ap.add_argument("--conversion-nonparallel", type=int, nargs="?", const=8, default=None, metavar="R",
                    help="with --conversion-train: TARGET.wav is other speech, not the same sentence; no alignment, up to "
                         "R rounds of nearest-row pairing and training, 1 to 50 (8)")
    ap.add_argument("--conversion-gv", type=float, nargs="?", const=0.25, default=None, metavar="S",
                    help="with --conversion-train and --conversion-span: store the target's global variance in the map, "
                         "with the relative spread S, 0 < S <= 10 (0.25); S is optional, so the flag must not stand directly "
                         "before the input file, which it would take for S")
    ap.add_argument("--conversion-no-gv", action="store_true",
                    help="with --conversion: leave the global-variance term out although the map carries it")
    ap.add_argument("--conversion-gv-iters", type=int, default=None, metavar="K",
                    help="with --conversion and a map that carries the global variance: sweeps, 0 to 10000 (30)")
    ap.add_argument("--conversion-gv-weight", type=float, default=None, metavar="G",
                    help="with --conversion and a map that carries the global variance: weight of the term, 1e-6 to 1e6 (1)")
    ap.add_argument("--conversion-em-iters", type=int, default=None, metavar="K",
                    help="with --conversion and a dynamic map: refine the mixture sequence by K EM iterations, 0 to 100, "
                         "before the global-variance term (convert.conversion_trajectory_em)")
    ap.add_argument("--conversion", default=None, metavar="MAP.npz",
                    help="also write <name>_modified.wav: amplitudes read off this file's cepstral envelope converted by "
                         "the map of a --conversion-train run; the pitch follows the target's statistics unless a "
                         "pitch flag is given")
    return ap


def load_conversion(path):
    """A --conversion-save file: (the validated map, order, lambda, fs, source (mean, std) of ln f0, target's).  The map
    holds cep_warp when the file does."""
    from .convert import check_conversion
    try:
        with np.load(path, allow_pickle=False) as z:
            d = {k: z[k] for k in z.files}
    except (OSError, ValueError) as e:
        raise ValueError("--conversion %s: cannot read the map (%s)" % (path, e)) from None
    conv = check_conversion(d)
    try:
        order, lam, fs = int(d["order"]), float(d["lam"]), int(d["fs"])
        src, tgt = (tuple(float(v) for v in d[k]) for k in ("src_f0", "tgt_f0"))
    except (KeyError, TypeError, ValueError):
        raise ValueError("--conversion %s: the file lacks order, lam, fs, src_f0 or tgt_f0" % path) from None
    dxs = conv["dx"] // 2 if "span" in conv else conv["dx"]       # a dynamic map counts the delta columns
    if len(src) != 2 or len(tgt) != 2 or order + 1 != dxs + (0 if conv["level"] else 1):
        raise ValueError("--conversion %s: the order and the f0 statistics do not fit the map" % path)
    return conv, order, lam, fs, src, tgt


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if a.noise_seed is not None and not a.noise:
        ap.error("--noise-seed needs --noise")
    if (a.pitch_jump_cost is not None or a.pitch_unvoiced is not None) and not a.pitch_viterbi:
        ap.error("--pitch-jump-cost and --pitch-unvoiced need --pitch-viterbi")
    if a.pitch_viterbi:   # reject bad values before the analysis runs
        from .pitch import _check_unvoiced, viterbi_costs
        try:
            viterbi_costs(3, **{k: v for k, v in viterbi_options(a).items() if k == "jump_cost"})
            _check_unvoiced(a.pitch_unvoiced, 1.0)
        except ValueError as e:
            ap.error("--pitch-viterbi: %s" % e)
    if a.noise_formant and not a.noise:
        ap.error("--noise-formant needs --noise")
    warped = a.formant_warp_curve is not None or a.formant_vtln is not None or a.formant_warp_from is not None
    if a.formant_count is not None:
        from .formant import FORMANT_TRACKS_MAX
        if a.formants_out is None and a.formant_warp_from is None:
            ap.error("--formant-count needs --formants-out or --formant-warp-from")
        if not 1 <= a.formant_count <= FORMANT_TRACKS_MAX:
            ap.error("--formant-count must be in [1, %d]" % FORMANT_TRACKS_MAX)
    if a.protect_transients and a.time_scale is None and a.time_scale_curve is None and a.timing_from is None:
        ap.error("--protect-transients needs --time-scale, --time-scale-curve or --timing-from")
    if a.transient_delta is not None:
        if not a.protect_transients and a.onsets_out is None:
            ap.error("--transient-delta needs --protect-transients or --onsets-out")
        from .transient import check_peak_arguments
        try:
            check_peak_arguments(delta=a.transient_delta)
        except ValueError as e:
            ap.error("--transient-delta: %s" % e)
    if a.noise_formant and a.formant_scale is None and a.formant_scale_curve is None and not warped:
        ap.error("--noise-formant needs --formant-scale, --formant-scale-curve, --formant-warp-curve or --formant-vtln")
    if a.formant_knee is not None and a.formant_vtln is None:
        ap.error("--formant-knee needs --formant-vtln")
    if a.noise_modulation is not None and not a.noise:
        ap.error("--noise-modulation needs --noise")
    if a.noise_cepstrum is not None and not a.noise:
        ap.error("--noise-cepstrum needs --noise")
    if a.noise_from is not None and not a.noise:
        ap.error("--noise-from needs --noise")
    if a.noise_from is not None and a.noise_modulation is not None:
        ap.error("--noise-from takes the other file's noise: not with --noise-modulation, which follows this file's pitch")
    if a.noise_from is not None and a.noise_cepstrum is None:
        a.noise_cepstrum = 63
    if a.noise_cepstrum is not None:
        from .cepstrum import _cepstrum_order
        _cepstrum_order(a.noise_cepstrum)
    if a.noise:
        from .args import _seed
        from .noise import _mod_harmonics
        _seed(0 if a.noise_seed is None else a.noise_seed)
        if a.noise_modulation is not None:
            _mod_harmonics(a.noise_modulation, "--noise-modulation")
    if a.no_envelope and (a.formant_scale is not None or a.formant_scale_curve is not None or warped):
        ap.error("the formant flags move the spectral envelope: not with --no-envelope")
    cepstral = a.cepstral_envelope is not None
    aligned = a.envelope_from is not None or a.timing_from is not None or a.noise_from is not None
    vocode = a.from_parameters is not None
    if a.cepstral_lambda is not None and not (cepstral or vocode or a.conversion_train is not None
                                              or a.conversion is not None):
        ap.error("--cepstral-lambda needs --cepstral-envelope, --from-parameters or a conversion flag")
    train, convert = a.conversion_train is not None, a.conversion is not None
    axis = 0.0
    if a.cepstral_warp is not None:
        if not (cepstral or vocode or a.envelope_from is not None or a.timing_from is not None or train or convert):
            ap.error("--cepstral-warp needs --cepstral-envelope, --from-parameters, --envelope-from, --timing-from, "
                     "--conversion-train or --conversion")
        axis = a.cepstral_warp
        if isinstance(axis, str):    # mel, bark: the coefficient depends on the file's sampling rate
            from .model import cepstrum_warp
            axis = cepstrum_warp(wavfile.read(a.wav)[0], axis)
    if vocode and a.no_envelope:
        ap.error("--from-parameters builds the model from its spectral envelope: not with --no-envelope")
    if cepstral and a.no_envelope:
        ap.error("--cepstral-envelope supplies the spectral envelope: not with --no-envelope")
    if a.envelope_from is not None and a.no_envelope:
        ap.error("--envelope-from supplies the spectral envelope: not with --no-envelope")
    if train != (a.conversion_save is not None):
        ap.error("--conversion-train and --conversion-save go together")
    if a.conversion_components is not None and not train:
        ap.error("--conversion-components needs --conversion-train")
    if a.conversion_span is not None and not train:
        ap.error("--conversion-span needs --conversion-train")
    if a.conversion_init is not None and not train:
        ap.error("--conversion-init needs --conversion-train")
    if a.conversion_nonparallel is not None:
        if not train:
            ap.error("--conversion-nonparallel needs --conversion-train")
        if not 1 <= a.conversion_nonparallel <= 50:
            ap.error("--conversion-nonparallel must be in [1, 50]")
    if train and convert:
        ap.error("--conversion applies a map, --conversion-train learns one: not together")
    if a.conversion_gv is not None and not (train and a.conversion_span is not None):
        ap.error("--conversion-gv needs --conversion-train and --conversion-span")
    tuned = a.conversion_gv_iters is not None or a.conversion_gv_weight is not None
    if (a.conversion_no_gv or tuned) and not convert:
        ap.error("--conversion-no-gv, --conversion-gv-iters and --conversion-gv-weight need --conversion")
    if a.conversion_no_gv and tuned:
        ap.error("--conversion-no-gv leaves the term out: not with --conversion-gv-iters or --conversion-gv-weight")
    if a.conversion_em_iters is not None and not convert:
        ap.error("--conversion-em-iters needs --conversion")
    if convert or a.conversion_gv is not None:
        from .convert import GV_MAX_ITERS, GV_REL_STD_MAX, GV_WEIGHT_RANGE
        if a.conversion_gv is not None and not 0 < a.conversion_gv <= GV_REL_STD_MAX:
            ap.error("--conversion-gv must be in (0, %g]" % GV_REL_STD_MAX)
        if a.conversion_gv_iters is not None and not 0 <= a.conversion_gv_iters <= GV_MAX_ITERS:
            ap.error("--conversion-gv-iters must be in [0, %d]" % GV_MAX_ITERS)
        if a.conversion_gv_weight is not None and not GV_WEIGHT_RANGE[0] <= a.conversion_gv_weight <= GV_WEIGHT_RANGE[1]:
            ap.error("--conversion-gv-weight must be in [%g, %g]" % GV_WEIGHT_RANGE)
    if convert and a.envelope_from is not None:
        ap.error("--conversion supplies the spectral envelope: not with --envelope-from")
    if convert and a.no_envelope:
        ap.error("--conversion supplies the spectral envelope: not with --no-envelope")
    if train:
        from .convert import DELTA_SPAN_RANGE, GMM_MAX_COMPONENTS
        if not 1 <= (8 if a.conversion_components is None else a.conversion_components) <= GMM_MAX_COMPONENTS:
            ap.error("--conversion-components must be in [1, %d]" % GMM_MAX_COMPONENTS)
        if a.conversion_span is not None and not DELTA_SPAN_RANGE[0] <= a.conversion_span <= DELTA_SPAN_RANGE[1]:
            ap.error("--conversion-span must be in [%d, %d]" % DELTA_SPAN_RANGE)
    cmap = None
    if convert:   # the map is read and checked before the analysis runs
        cmap = load_conversion(a.conversion)
        if a.cepstral_envelope and a.cepstral_envelope != cmap[1]:
            ap.error("--cepstral-envelope %d differs from the map's order %d" % (a.cepstral_envelope, cmap[1]))
        if a.cepstral_lambda is not None and a.cepstral_lambda != cmap[2]:
            ap.error("--cepstral-lambda %g differs from the map's %g" % (a.cepstral_lambda, cmap[2]))
        if a.cepstral_warp is not None and axis != cmap[0].get("cep_warp", 0.0):
            ap.error("--cepstral-warp %g differs from the map's %g" % (axis, cmap[0].get("cep_warp", 0.0)))
        if a.conversion_em_iters is not None:
            from .convert import EM_MAX_ITERS
            if not 0 <= a.conversion_em_iters <= EM_MAX_ITERS:
                ap.error("--conversion-em-iters must be in [0, %d]" % EM_MAX_ITERS)
            if "span" not in cmap[0]:
                ap.error("%s is a static map (--conversion-span when it was learned): not with --conversion-em-iters"
                         % a.conversion)
        if (a.conversion_no_gv or tuned) and "gv_mean" not in cmap[0]:
            ap.error("%s carries no global variance (--conversion-gv when it was learned): not with "
                     "--conversion-no-gv, --conversion-gv-iters or --conversion-gv-weight" % a.conversion)
    if a.align_band is not None and not (aligned or train):
        ap.error("--align-band needs --envelope-from, --timing-from, --noise-from or --conversion-train")
    if a.align_band is not None and not (np.isfinite(a.align_band) and a.align_band >= 0):
        ap.error("--align-band must be finite and >= 0")
    if cepstral or vocode:   # 0: the flag without a value, the default order
        from .cepstrum import _cepstrum_lambda, _cepstrum_order
        for order in (a.cepstral_envelope, a.from_parameters):
            if order:
                _cepstrum_order(order)
        _cepstrum_lambda(5e-4 if a.cepstral_lambda is None else a.cepstral_lambda)
    modify = any(x is not None for x in (a.time_scale, a.pitch_scale, a.time_scale_curve, a.pitch_scale_curve,
                                         a.formant_scale, a.formant_scale_curve)) or warped or cepstral or aligned or convert
    curves = {}
    wmap = None
    if modify or vocode:   # reject bad scales and curves before the analysis runs
        from .args import _scale
        _scale(1.0 if a.time_scale is None else a.time_scale, "--time-scale")
        _scale(1.0 if a.pitch_scale is None else a.pitch_scale, "--pitch-scale")
        _scale(1.0 if a.formant_scale is None else a.formant_scale, "--formant-scale")
        for key, path in (("time", a.time_scale_curve), ("pitch", a.pitch_scale_curve),
                          ("formant", a.formant_scale_curve)):
            if path is not None:
                curves[key] = read_scale_curve(path, "--%s-scale-curve %s" % (key, path))
        if a.formant_warp_curve is not None:
            wmap = read_warp_curve(a.formant_warp_curve, "--formant-warp-curve %s" % a.formant_warp_curve)
        if a.formant_vtln is not None:   # the map needs fs: the slopes are checked here, at the nominal fs = 2
            from .model import formant_warp_vtln
            formant_warp_vtln(2.0, a.formant_vtln, 0.875 if a.formant_knee is None else a.formant_knee)
    gender = a.gender
    if "," in gender:
        lo, hi = gender.split(",")
        gender = (float(lo), float(hi))
    analysis_options = dict(step=a.step, maxAdpt=a.max_adpt, pitchPeriods=a.pitch_periods,
                            analysisWindow=a.analysis_window, fullWaveform=not a.voiced_only, fc=a.fc,
                            partials=a.partials, printPrompts=True, loadingScreen=False,
                            track_budget_bytes=int(a.track_budget_mb * 2 ** 20) if a.track_budget_mb > 0 else "auto")
    if a.pitch_device:
        analysis_options["pitch_device"] = True
    if a.pitch_viterbi:
        analysis_options["pitch_viterbi"] = viterbi_options(a)
    on_axis = dict(cep_warp=axis) if axis != 0.0 else {}     # without the flag every call below is made without it
    s_recon, srer, det, t = analyse(a.wav, gender, analysis_options)
    if not a.no_write:
        fs, _ = wavfile.read(a.wav)
        out = a.wav[:len(a.wav) - 4] + "_reconstructed.wav"
        wavfile.write(out, fs, np.float32(s_recon))
        print("wrote", out)
        if a.formants_out is not None:
            write_formants(a.formants_out, *formant_table(a.wav, a.fc, a.formant_count or 3))
        onset_times = None
        if a.onsets_out is not None or a.protect_transients:
            onset_times, strength = onset_table(a.wav, a.fc, a.transient_delta)
            if a.onsets_out is not None:
                write_onsets(a.onsets_out, onset_times, strength)
        if train and a.conversion_nonparallel is not None:
            train_conversion_nonparallel(a, gender, analysis_options, fs, det, **on_axis)
        elif train:
            train_conversion(a, gender, analysis_options, fs, det, **on_axis)
        if modify or a.noise or vocode:
            from .model import eaQHMNoiseAnalysis, eaQHMNoiseModulation, eaQHMSynthesis, scale_contour
            rho = 1.0 if a.time_scale is None else a.time_scale
            beta = 1.0 if a.pitch_scale is None else a.pitch_scale
            if "time" in curves:
                rho = scale_contour(det, fs, *curves["time"])
            if "pitch" in curves:
                beta = scale_contour(det, fs, *curves["pitch"])
            alpha = 1.0 if a.formant_scale is None else a.formant_scale
            if "formant" in curves:
                alpha = scale_contour(det, fs, *curves["formant"])
            if a.formant_vtln is not None:
                from .model import formant_warp_vtln
                wmap = formant_warp_vtln(fs, a.formant_vtln, 0.875 if a.formant_knee is None else a.formant_knee)
            if a.formant_warp_from is not None:
                wmap = formant_warp_between(a.wav, a.formant_warp_from, a.fc, a.formant_count or 3, fs)
            nz = None
            if a.noise:
                from .prologue import read_signal
                sig = read_signal(a.wav, a.fc)[1]
                nz = eaQHMNoiseAnalysis(sig, s_recon, fs)
                if a.noise_modulation is not None:
                    nz = eaQHMNoiseModulation(sig, s_recon, nz, det, a.noise_modulation)
            ceps = None
            if cepstral or aligned:
                from .model import model_cepstrum
                order, lam = a.cepstral_envelope or None, 5e-4 if a.cepstral_lambda is None else a.cepstral_lambda
                ceps = model_cepstrum(det, fs, order, lam, **on_axis)
            if convert:   # this file's rows at the map's order and lambda, converted
                from . import convert as _convert
                from .convert import pitch_conversion_contour
                from .model import model_parameters
                conv, c_order, c_lam, fs_map, src_f0, tgt_f0 = cmap   # the alignment keeps its own order, lam
                if fs_map != fs:
                    raise ValueError("%s was learned at %d Hz, the input is sampled at %d Hz" % (a.conversion, fs_map, fs))
                synth_axis = dict(cep_warp=conv["cep_warp"]) if conv.get("cep_warp", 0.0) != 0.0 else {}
                p = model_parameters(det, fs, c_order, c_lam, **synth_axis)
                if "span" in conv and a.conversion_em_iters is not None:
                    converted = _convert.conversion_trajectory_em(conv, p["ceps"], em_iters=a.conversion_em_iters,
                                                                  **gv_options(a))
                elif "span" in conv:
                    converted = _convert.conversion_trajectory(conv, p["ceps"], **gv_options(a))
                else:
                    converted = _convert.conversion_apply(conv, p["ceps"])
                if a.pitch_scale is None and "pitch" not in curves:
                    beta = pitch_conversion_contour(p["f0"], p["voiced"] & (p["f0"] > 0), src_f0, tgt_f0)
            if aligned:
                from .model import alignment_index, alignment_time_scale, warp_rows
                others, n_inst = {}, len(ceps)
                for path in (a.envelope_from, a.timing_from, a.noise_from):
                    if path is not None and path not in others:
                        others[path] = align_other(path, gender, analysis_options, fs, ceps, order, lam,
                                                   2.0 if a.align_band is None else a.align_band,
                                                   a.fc if path == a.noise_from else None, **on_axis)
                if a.timing_from is not None:
                    rho = alignment_time_scale(others[a.timing_from][1], len(ceps))
                if a.envelope_from is not None:
                    C_other, pairs = others[a.envelope_from][:2]
                    ceps = warp_rows(C_other, alignment_index(pairs, len(ceps)))
                elif not cepstral:
                    ceps = None
                if a.noise_from is not None:   # OTHER's residual noise at this file's noise frames
                    from .model import noise_alignment_index, noise_cepstrum
                    pairs, det_o, nz_o = others[a.noise_from][1:]
                    j = noise_alignment_index(alignment_index(pairs, n_inst), det, nz, det_o, nz_o)
                    noise_rows = warp_rows(noise_cepstrum(nz_o, a.noise_cepstrum), j)
            if convert:
                ceps = converted
            if a.protect_transients:   # the same total length, the onsets at rate 1
                from .transient import protect_time_scale
                rho, kept = protect_time_scale(det, fs, len(s_recon), rho, onset_times, return_info=True)
                print("protected %d transients: the rest runs at %.4g x its time scale%s"
                      % (len(onset_times), kept["c"], ", %d instants clipped" % kept["clipped"] if kept["clipped"] else ""))
            if a.noise_cepstrum is not None:
                from .model import noise_cepstrum, noise_from_cepstrum
                if a.noise_from is None:
                    noise_rows = noise_cepstrum(nz, a.noise_cepstrum)
                kept = {k: nz[k] for k in ("mod", "mod_harmonics") if k in nz}
                nz = noise_from_cepstrum(noise_rows, nz["hop"], fs, order=nz["order"], length=nz["length"], **kept)
            common = dict(time_scale=rho, pitch_scale=beta, preserve_envelope=not a.no_envelope, formant_scale=alpha,
                          phase=a.phase, noise=nz, noise_seed=a.noise_seed or 0, noise_formant=a.noise_formant,
                          noise_modulation=a.noise_modulation is not None, formant_warp=wmap)
            if modify or a.noise:
                if not convert:          # the rows' axis: the flag's, or the map's
                    synth_axis = on_axis if ceps is not None else {}
                s_mod = eaQHMSynthesis(det, fs, len(s_recon), envelope=ceps, **synth_axis, **common)
                out = a.wav[:len(a.wav) - 4] + ("_modified.wav" if modify else "_resynthesis.wav")
                wavfile.write(out, fs, np.float32(s_mod))
                print("wrote", out)
            if vocode:   # the model reduced to arrays and rebuilt from them alone
                from .model import model_from_parameters, model_parameters
                p = model_parameters(det, fs, a.from_parameters or None,
                                     5e-4 if a.cepstral_lambda is None else a.cepstral_lambda, **on_axis)
                built = model_from_parameters(p["f0"], p["ceps"], p["fs"], p["step"], voiced=p["voiced"], **on_axis)
                s_voc = eaQHMSynthesis(built, fs, len(s_recon), **common)
                out = a.wav[:len(a.wav) - 4] + "_vocoded.wav"
                wavfile.write(out, fs, np.float32(s_voc))
                print("wrote", out)
    return 0


def formant_table(path, fc, n):
    """The formant tracks of a file's signal: formant.signal_allpole, formant_candidates and
    formant_tracks with their defaults.  Returns (fs, seconds float64[T], F float64[T, n], B float64[T, n])."""
    from . import formant
    from .prologue import read_signal
    fs, s = read_signal(path, fc)
    model = formant.signal_allpole(s, fs)
    F, B = formant.formant_tracks(formant.formant_candidates(model), n)
    return fs, np.arange(len(F)) * model["hop"] / float(fs), F, B


def write_formants(out, fs, seconds, F, B):
    """--formants-out: one line per frame, seconds, F1..FN, B1..BN."""
    n = F.shape[1]
    head = "seconds " + " ".join("F%d" % (i + 1) for i in range(n)) + " " + " ".join("B%d" % (i + 1) for i in range(n))
    np.savetxt(out, np.column_stack((seconds, F, B)), fmt="%.6f", header=head)
    print("wrote", out)


def onset_table(path, fc, delta=None):
    """The transient onsets of a file's signal: transient.onset_strength and transient.onsets with their
    defaults, the threshold `delta` unless None.  Returns (seconds float64[K], strength float64[K])."""
    from . import transient
    from .prologue import read_signal
    fs, s = read_signal(path, fc)
    on = transient.onsets(transient.onset_strength(s, fs), **({} if delta is None else dict(delta=delta)))
    return on["times"], on["strength"]


def write_onsets(out, seconds, strength):
    """--onsets-out: one line per onset, seconds and strength."""
    np.savetxt(out, np.column_stack((seconds, strength)).reshape(-1, 2), fmt="%.6f", header="seconds strength")
    print("wrote", out)


def formant_warp_between(path, other, fc, n, fs):
    """--formant-warp-from: the warp from `path`'s median formants to `other`'s, (f_in, f_out)."""
    from .formant import formant_warp_from_tracks
    fs_a, _, FA, _ = formant_table(path, fc, n)
    fs_b, _, FB, _ = formant_table(other, fc, n)
    if fs_b != fs_a:
        raise ValueError("%s is sampled at %d Hz, the input at %d Hz" % (other, fs_b, fs_a))
    f_in, f_out = formant_warp_from_tracks(FA, FB, fs)
    print("formant warp from %s: %s -> %s Hz" % (other, np.round(f_in, 1).tolist(), np.round(f_out, 1).tolist()))
    return f_in, f_out


def viterbi_options(a):
    """The arguments of pitch.analysis_pitch_track_viterbi that --pitch-jump-cost and --pitch-unvoiced set."""
    kw = {}
    if a.pitch_jump_cost is not None:
        kw["jump_cost"] = a.pitch_jump_cost
    if a.pitch_unvoiced is not None:
        kw["unvoiced"] = a.pitch_unvoiced
    return kw


def gv_options(a):
    """The global-variance arguments of conversion_trajectory that the flags set."""
    kw = {}
    if a.conversion_no_gv:
        kw["gv"] = False
    if a.conversion_gv_iters is not None:
        kw["gv_iters"] = a.conversion_gv_iters
    if a.conversion_gv_weight is not None:
        kw["gv_weight"] = a.conversion_gv_weight
    return kw


def conversion_init(a):
    """The init argument of conversion_train that --conversion-init sets: none for `axis`, today's start."""
    return dict(init="kmeans") if a.conversion_init == "kmeans" else {}


def train_conversion(a, gender, analysis_options, fs, det, **on_axis):
    """--conversion-train: analyses the target, aligns it to this file's model `det`, learns the map and saves it.
    on_axis is empty or cep_warp=a (--cepstral-warp): it reaches every fit and is stored in the map."""
    from .convert import conversion_pairs, conversion_train, f0_statistics, gv_statistics
    from .model import model_parameters
    order, lam = a.cepstral_envelope or None, 5e-4 if a.cepstral_lambda is None else a.cepstral_lambda
    p = model_parameters(det, fs, order, lam, **on_axis)
    C_t, pairs, det_t, _ = align_other(a.conversion_train, gender, analysis_options, fs, p["ceps"], order, lam,
                                       2.0 if a.align_band is None else a.align_band, **on_axis)
    X, Y = conversion_pairs(p["ceps"], C_t, pairs, a.conversion_span)
    gv = None if a.conversion_gv is None else gv_statistics([C_t], rel_std=a.conversion_gv)
    conv = conversion_train(X, Y, 8 if a.conversion_components is None else a.conversion_components,
                            span=a.conversion_span, gv=gv, **conversion_init(a))
    p_t = model_parameters(det_t, fs, order, lam, **on_axis)
    stats = [f0_statistics(q["f0"], q["voiced"] & (q["f0"] > 0)) for q in (p, p_t)]
    np.savez(a.conversion_save, order=np.int64(p["ceps"].shape[1] - 1), lam=np.float64(lam), fs=np.int64(fs),
             src_f0=np.array(stats[0]), tgt_f0=np.array(stats[1]), **{k: np.float64(v) for k, v in on_axis.items()},
             **conv)
    print("wrote %s: %d pairs, %d components, mean log-likelihood %g"
          % (a.conversion_save, len(X), len(conv["weights"]), conv["loglik"][-1]))


def train_conversion_nonparallel(a, gender, analysis_options, fs, det, **on_axis):
    """--conversion-train with --conversion-nonparallel: analyses the target, fits both cepstra, learns the map without an
    alignment (nonparallel.conversion_train_nonparallel) and saves train_conversion's fields.  With --conversion-span the
    dynamic map is trained from the pairs of the returned map."""
    from . import convert, nonparallel
    from .model import model_cepstrum, model_parameters
    order, lam = a.cepstral_envelope or None, 5e-4 if a.cepstral_lambda is None else a.cepstral_lambda
    p = model_parameters(det, fs, order, lam, **on_axis)
    fs_t, _ = wavfile.read(a.conversion_train)
    if fs_t != fs:
        raise ValueError("%s is sampled at %d Hz, the input at %d Hz" % (a.conversion_train, fs_t, fs))
    _, _, det_t, _ = analyse(a.conversion_train, gender, analysis_options)
    C_t = model_cepstrum(det_t, fs, order, lam, **on_axis)
    M = 8 if a.conversion_components is None else a.conversion_components
    conv, info = nonparallel.conversion_train_nonparallel(p["ceps"], C_t, M, rounds=a.conversion_nonparallel,
                                                          **conversion_init(a))
    print("paired %s without an alignment: %d pairs after %d rounds, mean squared distance %g -> %g"
          % (a.conversion_train, len(info["ix"]), info["rounds"], info["trace"][0], info["trace"][info["best"]]))
    if a.conversion_span is not None:
        gv = None if a.conversion_gv is None else convert.gv_statistics([C_t], rel_std=a.conversion_gv)
        X, Y = (convert.dynamic_rows(C, a.conversion_span)[i] for C, i in ((p["ceps"], info["ix"]), (C_t, info["iy"])))
        conv = convert.conversion_train(X, Y, M, span=a.conversion_span, gv=gv, **conversion_init(a))
    p_t = model_parameters(det_t, fs, order, lam, **on_axis)
    stats = [convert.f0_statistics(q["f0"], q["voiced"] & (q["f0"] > 0)) for q in (p, p_t)]
    np.savez(a.conversion_save, order=np.int64(p["ceps"].shape[1] - 1), lam=np.float64(lam), fs=np.int64(fs),
             src_f0=np.array(stats[0]), tgt_f0=np.array(stats[1]), **{k: np.float64(v) for k, v in on_axis.items()},
             **conv)
    print("wrote %s: %d pairs, %d components, mean log-likelihood %g"
          % (a.conversion_save, len(info["ix"]), len(conv["weights"]), conv["loglik"][-1]))


def align_other(path, gender, analysis_options, fs, ceps, order, lam, band_s, noise_fc=None, **on_axis):
    """Analyses `path` with the same options, fits its cepstrum (on the axis of `ceps`: on_axis is empty or cep_warp=a)
    and aligns it to `ceps`: (its cepstrum, the path, its model, and with `noise_fc` (the --fc of the analysis) the noise
    model of its residual, else None)."""
    from .model import band_min_radius, eaQHMNoiseAnalysis, model_align, model_cepstrum, unpack_model
    fs_o, _ = wavfile.read(path)
    if fs_o != fs:
        raise ValueError("%s is sampled at %d Hz, the input at %d Hz" % (path, fs_o, fs))
    s_recon_o, _, det_o, _ = analyse(path, gender, analysis_options)
    C_o = model_cepstrum(det_o, fs, order, lam, **on_axis)
    r = max(int(round(band_s * fs / unpack_model(det_o)["step"])), band_min_radius(len(ceps), len(C_o)))
    pairs, cost = model_align(ceps, C_o, band=r)
    print("aligned %s: %d pairs, cost %g" % (path, len(pairs), cost))
    nz_o = None
    if noise_fc is not None:
        from .prologue import read_signal
        nz_o = eaQHMNoiseAnalysis(read_signal(path, noise_fc)[1], s_recon_o, fs)
    return C_o, pairs, det_o, nz_o


def _two_columns(path, name, what):
    try:
        xy = np.loadtxt(path, comments="#", ndmin=2)
    except (OSError, ValueError) as e:
        raise ValueError("%s: cannot read two numeric columns (%s)" % (name, e)) from None
    if xy.shape[1] != 2:
        raise ValueError("%s: expected two columns (%s), got %d" % (name, what, xy.shape[1]))
    return xy[:, 0], xy[:, 1]


def read_scale_curve(path, name):
    """A breakpoint curve file: (times, values), validated as model.check_curve does."""
    from .model import check_curve
    return check_curve(*_two_columns(path, name, "seconds, value"), name)


def read_warp_curve(path, name):
    """A formant warp file, lines 'Hz_in Hz_out': (f_in, f_out), validated as model.check_formant_warp does."""
    from .args import _warp_rows
    try:
        f_in, f_out = _warp_rows(_two_columns(path, name, "Hz in the model, Hz in the output"), 1, "file")
    except ValueError as e:
        raise ValueError("%s: %s" % (name, e)) from None
    return f_in, f_out[0]
