/* eaqhm_hip.h — C ABI of libeaqhm_hip.so: the MI355X (gfx950) implementation of the eaQHM per-frame
 * analysis hot path.
 *
 * The reference (Antibas/eaQHM-analysis-and-synthesis-in-Python) has no FFI: its boundary for this path
 * is the Python function eaQHMAnalysisAndSynthesis (functions.py:35-418) and the inner seams
 * iqhmLS_complexamps (functions.py:420-470), eaqhmLS_complexamps (functions.py:472-535) and
 * phase_integr_interpolation (functions.py:537-575).  Each entry point below names the reference lines
 * it replaces.  The host side (Python, ctypes) lives in eaqhm-analysis-and-synthesis-in-python_amd/.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name starts with h_ (host); buffers are owned by the
 *    caller (the Python host allocates them as torch-ROCm tensors and passes tensor.data_ptr());
 *  - all work is enqueued on the stream given to eaqhm_set_stream (a hipStream_t passed as void*;
 *    NULL = the default stream) and is asynchronous; eaqhm_sync waits for it;
 *  - every function returns 0 on success or a negative EAQHM_E* code; eaqhm_last_error gives the text;
 *    nothing throws, nothing frees caller memory;
 *  - floating point is IEEE double everywhere (the reference is float64/complex128 throughout).
 *
 * Layouts ("harmonic-major" = the reference's (L, Kmax) arrays transposed so time is contiguous)
 *  - s, target, s_hat       double[L]
 *  - am_cur, fm_cur         double[Kmax][track_len] dense tracks of the previous adaptation (functions.py:159-160,
 *                                                   :337-338, :375, :383) for the samples [track_t0, track_t0 +
 *                                                   track_len) of the file: the whole file (0, L), one rank's time
 *                                                   range plus halo, or one time block of a long file (the reference
 *                                                   keeps seven such (L, Kmax) arrays resident).  A frame window
 *                                                   [c-wl-1, c+wl] handed to eaqhm_ls_batch must lie inside it.
 *  - records                double[No_ti][3*Kmax+1] one row per analysis instant: |a_k| (Kmax), f_k (Kmax),
 *                                                   arg a_k (Kmax) written at functions.py:316-324, then the
 *                                                   DC term a0 (functions.py:303).  Rows of one contiguous
 *                                                   range of instants are one contiguous block, which is what
 *                                                   the per-adaptation all-gather across GPUs moves.
 *  - frame tables           one entry per ANALYSED frame (functions.py:180-181 true), ascending in time
 */
#ifndef EAQHM_HIP_H
#define EAQHM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EAQHM_OK 0
#define EAQHM_EINVAL (-1)  /* bad argument (shape / range)        */
#define EAQHM_EHIP (-2)    /* a HIP runtime call failed            */
#define EAQHM_ENOMEM (-3)  /* scratch allocation failed            */

typedef struct eaqhm_ctx eaqhm_ctx;

/* life cycle ------------------------------------------------------------------------------------ */
int eaqhm_ctx_create(eaqhm_ctx** out, int device);
int eaqhm_ctx_destroy(eaqhm_ctx* ctx);
int eaqhm_set_stream(eaqhm_ctx* ctx, void* hip_stream);
int eaqhm_sync(eaqhm_ctx* ctx);
const char* eaqhm_last_error(eaqhm_ctx* ctx);
/* tuning knobs (for A/B measurements; defaults are the fastest validated choice)
 *   EAQHM_OPT_LS_VARIANT: 2 = MFMA Gramian + tile Cholesky through memory for every frame (the large-frame kernel),
 *                         3 = Gramian and tile Cholesky on chip for frames of <= 13 tile rows (Kc <= 103), the
 *                             large-frame kernel for the rest (default) */
#define EAQHM_OPT_LS_VARIANT 1
#define EAQHM_OPT_DEBUG_KEEP 2   /* 1: accumulate the in-kernel phase stamps across launches; 2: also time diag_D */
#define EAQHM_OPT_DTW_PHASES 3   /* measurements: 1 = eaqhm_dtw launches its forward pass only, 2 = its backtrack only
                                    (on a band that holds D and a ptr that is filled), 0 = both (default) */
/*   EAQHM_OPT_A0_RESIDENT (an addition under ABI 6): 1 = the adaptation-0 frames of <= 13 tile rows are solved by a kernel
 *                         of their own, two workgroups resident per CU, when the launch's wl_max and Kmax let its LDS
 *                         fit 80 KiB (default; the records are bitwise those of 0), 0 = by the tile kernel, as a launch
 *                         that does not fit is.  With EAQHM_OPT_DEBUG_KEEP on, word 15 of eaqhm_debug_read counts the
 *                         frames that kernel solved. */
#define EAQHM_OPT_A0_RESIDENT 4
int eaqhm_set_option(eaqhm_ctx* ctx, int32_t key, int32_t value);
/* diagnostics: shader-clock cycles per phase of the LS tile kernel summed over frames (thread 0 of each
 * workgroup): {setup, basis build, contraction, factorisation total..., see csrc/eaqhm_ls_tile.hip STAMP} */
int eaqhm_debug_read(eaqhm_ctx* ctx, uint64_t h_out[16]);
/* singular systems: the reference aborts with numpy.linalg.LinAlgError from inv() when a frame's normal matrix is
 * singular — an exactly zero LU pivot (functions.py:465, :530); an ill-conditioned system is solved and returned.  The
 * kernels factorise by Cholesky; what corresponds to the exact zero is a BREAKDOWN of the factorisation: a pivot that
 * is not positive or has fallen to <= 2.5e-13 (order x eps) of its original diagonal entry, as two identical basis
 * columns give.  Such frames are counted in a device counter (h_count[0]); ill-conditioned but factorisable systems are
 * solved like the reference solves them.  h_count[1] counts diagonal-tile pipelines whose internal hand-shake timed
 * out — never nonzero unless the library has a bug; the host raises RuntimeError for it, LinAlgError for h_count[0].
 * h_count[2] counts frames whose analysis window [c-wl-1, c+wl] was not inside the signal / the resident track window
 * handed to eaqhm_ls_batch: such a frame is dropped (its record row is not written) instead of being read out of bounds;
 * the host raises ValueError.  eaqhm_ls_faults waits for the stream, returns the counts since the last read and clears
 * them; eaqhm_eval_synth also reports (and clears) them in sums_out[4..6], so the adaptation loop needs no extra
 * device->host read. */
int eaqhm_ls_faults(eaqhm_ctx* ctx, int32_t h_count[3]);
/* library / device facts: fills {n_cu, lds_bytes, clock_khz, abi_version} */
int eaqhm_device_info(eaqhm_ctx* ctx, int32_t h_info[4]);

/* adaptation >= 1 frame set-up ---------------------------------------------------------------------
 * Replaces functions.py:202-213: the active-slot list of each frame (indices of nonzero
 * fm_current[c,:]) and the empty-row seeding flag (slot 0 <- 140 Hz / 10e-4).  The seeding WRITE of the
 * reference is not performed: `seeded[c]` (uint8[L], zeroed here) marks the rows and the LS kernel
 * applies "visible to frames at or after c" itself, which reproduces the sequential loop exactly.
 *   ncol[f]            number of active slots of frame f
 *   cols[f*Kmax + j]   j-th active slot (ascending)
 *   any_seed           int32[1], nonzero if any frame was seeded                                     */
int eaqhm_frame_prep(eaqhm_ctx* ctx, const double* fm_cur, int64_t L, int64_t track_t0, int64_t track_len, int32_t Kmax,
                     const int32_t* frame_c, int32_t n_frames, int32_t* ncol, int32_t* cols, uint8_t* seeded,
                     int32_t* any_seed);

/* the per-frame least squares, batched over frames ---------------------------------------------------
 * Replaces, for every analysed frame of one adaptation:
 *   adaptation 0 (mode 0): functions.py:187-197 + iqhmLS_complexamps (functions.py:420-470)
 *   adaptation>=1 (mode 1): functions.py:244-295 (track windows, zero-gap fill, negative/DC/positive
 *                           column layout) + eaqhmLS_complexamps (functions.py:472-535)
 *   both: frequency correction (functions.py:297), slot scatter (:299-301), acceptance test and
 *         frame-centre writes (:303-324).
 * Inputs
 *   frame_inst[f] instant index i (row of the records), frame_c[f] 0-based centre sample (tith-1),
 *   frame_wl[f] half window length (functions.py:191), frame_f0[f] / frame_K[f] adaptation-0 pitch and
 *   harmonic count (functions.py:185-187; ignored in mode 1), ncol/cols/seeded/any_seed from
 *   eaqhm_frame_prep (mode 1; may be NULL in mode 0), wl_max >= max(frame_wl) (sizes the per-workgroup
 *   scratch), a_iter the adaptation number (h = f0/(a+1),
 *   functions.py:310), f0_stale the pitch of the last frame of adaptation 0 (used for every frame when
 *   a_iter >= 1, functions.py:310/:321 quirk), f0min (functions.py:321).
 * Outputs
 *   records[i][...] for the frames' instants (the whole row of 3*Kmax+1 values is written),
 *   optional raw_amp / raw_slope: double[n_frames][2*(2*Kmax+1)] interleaved complex LS solutions in
 *   column order [negative block | DC | positive block] (NULL to skip) — what the two seam functions
 *   return.                                                                                           */
int eaqhm_ls_batch(eaqhm_ctx* ctx, int32_t mode, const double* s, int64_t L, double fs, const double* am_cur,
                   const double* fm_cur, int64_t track_t0, int64_t track_len, int32_t Kmax,
                   const int32_t* frame_inst, const int32_t* frame_c,
                   const int32_t* frame_wl, const double* frame_f0, const int32_t* frame_K, const int32_t* ncol,
                   const int32_t* cols, const uint8_t* seeded, const int32_t* any_seed, int32_t n_frames,
                   int32_t wl_max, int32_t a_iter, double f0_stale, double f0min, double* records, double* raw_amp,
                   double* raw_slope);

/* the two LS seams with explicit matrices, one frame ------------------------------------------------
 * eaqhm_ls_explicit: eaqhmLS_complexamps(s, am, fm, window, fs) (functions.py:472-535) when `fm` is
 * non-NULL — am, fm are double[N][Kc] row-major; iqhmLS_complexamps(s, f0range, window, fs)
 * (functions.py:420-470) when `fm` is NULL and `f0range` (double[Kc]) is given.
 * out_amp / out_slope: double[2*Kc] interleaved complex.                                            */
int eaqhm_ls_explicit(eaqhm_ctx* ctx, const double* s, int32_t N, const double* am, const double* fm,
                      const double* f0range, int32_t Kc, const double* window, double fs, double* out_amp,
                      double* out_slope);

/* the third inner seam, stand-alone ---------------------------------------------------------------
 * phase_integr_interpolation(fm_recon, ph_recon, indices) (functions.py:537-575): `omega` = 2*pi/fs * fm_recon
 * and `ph` are dense columns, `knots` (int32[n_knots], ascending, any spacing) the knot samples with
 * first = knots[0], last = knots[n_knots-1]; out = double[last-first+1], the dense phase on [first, last]. */
int eaqhm_phase_integrate(eaqhm_ctx* ctx, const double* omega, const double* ph, const int32_t* knots,
                          int32_t n_knots, int32_t first, int32_t last, double* out);

/* interpolation stage 1: segments + spline systems ---------------------------------------------------
 * Replaces the knot bookkeeping and the not-a-knot cubic solves of functions.py:340 (a0, all instants)
 * and :346-371 (per harmonic: runs of consecutive accepted instants, cubic through the knots).
 *   code[i][k]  uint8: 0 not accepted, 1 isolated accepted instant, 2 member of a run of >= 4 knots,
 *               16 + 4*m + pos for runs of m = 2 or 3 knots (pos = position inside the run)
 *   mom[i][k]   double[No_ti][Kmax+1] second derivatives of the fm splines (column Kmax: the a0 spline) */
int eaqhm_spline_solve(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, int32_t step,
                       uint8_t* code, double* mom);
/* the same for the instants [i_lo, i_hi) only (a rank that evaluates only its own time range: the moments are
 * local sums, so the rest of `code` / `mom` is neither read nor written, except the run codes of instants 0..3) */
int eaqhm_spline_solve_range(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, int32_t step,
                             int32_t i_lo, int32_t i_hi, uint8_t* code, double* mom);

/* interpolation stage 2 + synthesis + SRER -----------------------------------------------------------
 * Replaces functions.py:364 (linear am), :367-371 (cubic fm, incl. the <4-knot padded case),
 * :373 + phase_integr_interpolation (functions.py:537-575), :375 (next-iteration frequency from the
 * unwrapped phase), :383 (am_current), :385 (additive synthesis) and :388 (SRER).
 * Samples [t_lo, t_hi) are produced (the whole signal when 0, L); the error sums cover [s_lo, s_hi)
 * inside that range (a rank of a time-sharded run produces its range plus a halo but sums only its own).
 *   am_out, fm_out   double[Kmax][track_len]: next adaptation's am_current / fm_current for the samples
 *                    [track_t0, track_t0 + track_len) >= [t_lo, t_hi); both NULL: no track output (a long file's
 *                    synthesis pass: its tracks are regenerated block by block from the records)
 *   ph_knot          double[No_ti][Kmax] dense phase at the instants (what functions.py:411 packs)
 *   s_hat            double[L]; NULL: tracks only — no synthesis, no ph_knot, no error sums (target, ph_knot,
 *                    partials, sums_out may then be NULL too)
 *   partials         8-byte words, eaqhm_eval_partials_len of them: per-block error sums
 *   sums_out         double[16]: {sum d, sum d^2, n, SRER dB, LS breakdowns, stalled pipelines and dropped frames since the
 *                    last read (see eaqhm_ls_faults), -, then eight int64 bit patterns} with d = target - s_hat over
 *                    [s_lo,s_hi).  The int64 words are the same sums in fixed point, which add up exactly over blocks,
 *                    ranks and time blocks, so the SRER (functions.py:388, the input of the stop rule :394) does not
 *                    depend on how the file was split; sums_out[3] is that SRER for this call's range alone.
 *                    The fixed point follows the level of the signal.  std_det (functions.py:161, the same number on
 *                    every rank) = m 2^e with 0.5 <= m < 1 gives the shift s = 10 - e (0 when std_det is zero or not
 *                    finite; clamped to +-900), so that std_det 2^s lies in [2^9, 2^10), and d' = d 2^s is what is
 *                    summed:
 *                      words 0..2  three signed base-2^32 limbs of sum rint(d' 2^60)
 *                      words 3..5  three of sum rint(d'^2 2^64), d'^2 rounded to double first
 *                      word  6     the number of samples with |d'| >= 2^30 or d not finite; they enter no sum, and
 *                                  the SRER is NaN when there is one
 *                      word  7     s: the words say at which scale they were taken (s = 0: plain d 2^60, d^2 2^64).
 *                                  Every call writes it; a host that adds the words of several ranks leaves it out
 *                                  of the sum and keeps one copy
 *                    rint is to nearest, ties to even.  Representable: a single error up to 2^20 times the signal's
 *                    own level (a click 120 dB above it) in steps of 2^-70 of that level, its square in steps of
 *                    2^-84 of the squared level: an SRER of 180 dB is still resolved to 1e-7 dB.  The top limb of one
 *                    sample is below 2^60; the int64 sums hold sum d'^2 < 2^63, that is n x (mean square error /
 *                    std_det^2) < 2^43: 2^23 samples at an SRER of -60 dB, 2^43 at 0 dB.
 *                    sum d = (w0 + w1 2^32 + w2 2^64) 2^-60 2^-s, sum d^2 = (w3 + w4 2^32 + w5 2^64) 2^-64 2^-2s.    */
int eaqhm_eval_synth(eaqhm_ctx* ctx, const double* records, const uint8_t* code, const double* mom,
                     int32_t No_ti, int32_t Kmax, int32_t step, double fs, int64_t L, int64_t t_lo, int64_t t_hi,
                     int64_t s_lo, int64_t s_hi, const double* target, double std_det, double* am_out,
                     double* fm_out, int64_t track_t0, int64_t track_len, double* ph_knot, double* s_hat,
                     double* partials, double* sums_out);
/* number of 8-byte words `partials` must hold for a given range: eight per evaluation block.  Blocks hold at least 16
 * samples and sit on a grid fixed to sample 0 (to the analysis instants where the step allows), so a range of n samples
 * touches at most ceil(n / 16) + 1 of them, and that is what is counted */
int64_t eaqhm_eval_partials_len(int64_t t_lo, int64_t t_hi, int32_t step);

/* resynthesis from the model with a time scale rho, a pitch scale beta and a formant scale alpha (ABI 4) ----------
 * Generalises functions.py:337-385 (track interpolation and additive synthesis) and :537-575 (phase integration) from
 * the analysed timeline to output samples n' = rho * tau; the definition is DESIGN.md "Resynthesis from the model"
 * (§9), §9.1 for scales per analysis instant (contours), §9.2 for the formant scale and §11 for the
 * shape-invariant phase.  All calls take the records
 * of an analysed (possibly edited) model and the code / mom that eaqhm_spline_solve produced from them; at
 * rho = beta = 1 the synthesis is eaqhm_eval_synth's s_hat of the same records.
 * eaqhm_modify_prep (kernels: prep, segmented scan of the phase increments) serves every synthesis:
 *   beta       double[No_ti]    pitch scale per instant (the scalar synthesis passes No_ti equal values)
 *   gain       double[No_ti-1]  g_j of the contour map below, or NULL: Delta unweighted (the scalar map, and the shape
 *                               phase on either map)
 *   alpha      double[No_ti]    formant scale per instant, each finite and > 0, or NULL: no formant scale; it needs
 *                               preserve_envelope != 0
 *   amp        double[No_ti][Kmax]  knot amplitudes A': beta_i == 1 and alpha_i == 1: |a|; otherwise, with
 *                                   preserve_envelope, exp(E_i((beta_i * f) / alpha_i)), without it |a|; zero where
 *                                   beta_i * f >= fs/2 (the output frequency; alpha plays no part) or the slot is
 *                                   inactive.  E_i is the piecewise-linear envelope of ln |a| over the instant's
 *                                   active slots sorted by (f, k) (flat outside the end nodes, the first of tied nodes
 *                                   at a node's own frequency); a feature at F in the model sits at alpha_i F after
 *                                   the scale.  The nodes are ordered in LDS (3 * Kmax doubles per instant, four
 *                                   instants per block).
 *   R          double[No_ti][Kmax]  unwrapped knot phase along each run of consecutive active instants (0 at the run's
 *                                   first knot, R_{j+1} = R_j + (ph_{j+1} - ph_j) + 2 pi M_j); 0 outside runs.  With
 *                                   gain it is the weighted knot phase G, G_{j+1} = G_j + g_j ((ph_{j+1} - ph_j) +
 *                                   2 pi M_j).
 *   ph0        double[No_ti][Kmax]  phase of the first knot of the run each knot belongs to; 0 outside runs
 * eaqhm_modify_synth (kernels: one eval kernel per combination of the two groups below) writes out[t_lo, t_hi) of the
 *   L_out-sample signal (out is double[L_out]) from the outputs of a prep.  Two optional groups of arguments, each
 *   given whole or not at all (NULL pointers), select the time map and the phase:
 *   C, rate, gain, rate_min   all NULL: the scalar map tau = n'/rho with phase weight beta rho, from a prep without
 *                             gain; rho is the time scale, beta the number the prep's beta array holds; rate_min is not
 *                             read.  All given: the contour map of §9.1, and rho, beta are not read.  Per interval j:
 *                             r_j = (rho_j + rho_{j+1}) / 2, b_j = (beta_j + beta_{j+1}) / 2, g_j = r_j b_j; output
 *                             knots C_0 = 0, C_{j+1} = C_j + r_j step (the caller computes them in double, in this
 *                             order); L_out = rint(C_{n-1} + rho_{n-1} (L - c_{n-1})).  C[No_ti] output knot positions,
 *                             rate[No_ti] = r_j with rate[No_ti-1] = rho_{n-1} (past the last knot), gain[No_ti-1] =
 *                             g_j, rate_min = the smallest entry of rate (sizes the staged rows).  The prep ran with
 *                             this gain, unless f0, S are given.
 *   f0, S                     both NULL: every slot's phase is scaled on its own.  Both given: the shape-invariant
 *                             phase of §11, from a prep WITHOUT gain (R unweighted) on either map.
 *                             f0[No_ti] is the fundamental track in Hz (finite, >= 0), linear between instants;
 *                             S[No_ti] the fundamental's phase advance in cycles at each instant, in [0, 1): S_0 = 0,
 *                             S_{j+1} = frac(S_j + (g_j - 1) (step / fs) (f0_j + f0_{j+1}) / 2), computed by the caller
 *                             in double in this order, g_j = beta rho on the scalar map and gain[j] on the contour map.
 *                             The phase of slot k at an output sample in interval j at offset r is ph0 + R_j + Psi_j(r)
 *                             + 2 pi (k+1) (S_j + (g_j - 1) (f0_j r + (f0_{j+1} - f0_j) r^2 / (2 step)) / fs);
 *                             amplitudes, isolated knots and a0 are those of the independent phases.  With every
 *                             g_j = 1 and S = 0 the result is that of the same map without f0, S.
 * eaqhm_model_envelope (kernel: one wave per instant, lanes over the grid)
 *   out        double[No_ti][F]  E_i(freqs[t] / alpha_i), the natural-log amplitude, not muted; -inf on the rows of
 *                                instants without active slots.  freqs[F] is the caller's grid (device, finite, >= 0).
 * Device arrays are the caller's: every beta, alpha and rate must be finite and > 0 and C strictly increasing.
 * EAQHM_EINVAL for null pointers (other than gain and alpha of the prep and the two groups of the synthesis), a group
 * given in part, No_ti < 4, alpha without preserve_envelope, rho or beta (scalar map) or rate_min (contour map) <= 0 or
 * not finite, a range outside [0, L_out), F <= 0, and Kmax beyond the LDS budget of the envelope nodes (Kmax > 1706). */
int eaqhm_modify_prep(eaqhm_ctx* ctx, const double* records, const uint8_t* code, const double* mom, int32_t No_ti,
                      int32_t Kmax, int32_t step, double fs, const double* beta, const double* gain,
                      const double* alpha, int32_t preserve_envelope, double* amp, double* R, double* ph0);
int eaqhm_modify_synth(eaqhm_ctx* ctx, const double* records, const uint8_t* code, const double* mom, const double* amp,
                       const double* R, const double* ph0, int32_t No_ti, int32_t Kmax, int32_t step, double fs,
                       double rho, double beta, int64_t L_out, int64_t t_lo, int64_t t_hi, double* out, const double* C,
                       const double* rate, const double* gain, double rate_min, const double* f0, const double* S);
int eaqhm_model_envelope(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, const double* alpha,
                         const double* freqs, int32_t F, double* out);

/* the stochastic component: an LPC model of the residual and its resynthesis as filtered noise (ABI 5) -----------------
 * Not in the reference; the definition is DESIGN.md "The stochastic component" (§10).  hop = H, order = p,
 * 1 <= hop <= 1024, 1 <= order <= 63, order < 4 hop.
 * eaqhm_noise_analyse (kernel: one wave per frame, the windowed frame in LDS, lane l owns lag l, Levinson-Durbin in the
 *   wave) models e = s - s_recon (double[L]) in frames m = 0 .. Nf-1, Nf = (L-1)/hop + 1, centred at m hop, 4 hop long:
 *   sigma      double[Nf]         standard deviation of the white excitation; 0 for a silent frame
 *   refl       double[Nf][order]  reflection coefficients k_1..k_p of A(z); zeros from the first |k_i| >= 1 on
 * eaqhm_noise_synth (kernels: all-pole lattice, one lane per output frame; cross-fade of the two frames covering a
 *   sample) writes out[t_lo, t_hi) of the L_out-sample noise signal (out is double[L_out]); accumulate != 0 adds it to
 *   what out holds instead.  The excitation is a pure function of (seed, sample index), so the result does not depend
 *   on how [0, L_out) is split into ranges.
 *   tau        double[Nq]         Nq = (L_out-1)/hop + 1: the position, in samples of the analysed signal, that output
 *                                 frame centre q hop maps back to (finite, >= 0); sigma and refl are interpolated
 *                                 linearly between frames floor(tau/hop) and the next, held past the last frame
 *   mod, harmonics, theta, nu     an optional group (ABI 6): the three pointers all NULL give the plain cross-fade, and
 *                                 harmonics is not read; all given, the pitch-synchronous modulation of §10.2 (below)
 * EAQHM_EINVAL for null pointers (other than that group), the group given in part, harmonics outside [1, 8] with it,
 * L < 1, Nf < 1, hop or order outside the limits above, Nq != (L_out-1)/hop + 1 and a range outside [0, L_out).      */
int eaqhm_noise_analyse(eaqhm_ctx* ctx, const double* e, int64_t L, int32_t hop, int32_t order, double* sigma,
                        double* refl);
int eaqhm_noise_synth(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf, int32_t hop, int32_t order,
                      const double* tau, int32_t Nq, uint64_t seed, int64_t L_out, int64_t t_lo, int64_t t_hi,
                      double* out, int32_t accumulate, const double* mod, int32_t harmonics, const double* theta,
                      const double* nu);

/* the formant warp of the noise model (additions under ABI 5) ----------------------------------------
 * A frame (sigma, k_1..k_p) is the power spectrum P(w) = sigma^2 / |A(e^{jw})|^2, A the step-up of k.
 * eaqhm_noise_warp (kernel: one wave per frame; the spectrum at min(w_t / alpha, pi) on the grid w_t = pi t / 1024,
 *   t = 0..1024, in LDS; lane l owns lag l of its autocorrelation; the Levinson-Durbin recursion of the analysis) gives
 *   the model whose spectrum is the frame's moved up in frequency by alpha[m]:
 *   sigma_out  double[Nf]         sqrt(E) of the refit; a frame with alpha == 1 is copied bit for bit, a silent frame
 *   refl_out   double[Nf][order]  (sigma == 0) gives sigma_out = 0 and zeros
 * eaqhm_noise_envelope (kernel: one wave per frame, lanes over the grid) reads the warped spectrum itself:
 *   out        double[Nf][F]      2 ln sigma_m - 2 ln |A_m(e^{jw})| at w = 2 pi min(fnorm[t] / alpha[m], 1/2), fnorm =
 *                                 f / fs (device, finite, >= 0); -inf on the rows of silent frames
 * alpha[Nf] is the caller's: finite and > 0.  EAQHM_EINVAL for null pointers, Nf < 1, F < 1, order outside [1, 63].    */
int eaqhm_noise_warp(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf, int32_t order,
                     const double* alpha, double* sigma_out, double* refl_out);
int eaqhm_noise_envelope(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf, int32_t order,
                         const double* alpha, const double* fnorm, int32_t F, double* out);

/* pitch-synchronous modulation of the noise (additions under ABI 5) ----------------------------------
 * The noise of voiced speech comes in bursts locked to the glottal cycle.  Per noise frame the power envelope over the
 * fundamental's phase theta (cycles) is g^2(theta) = 1 + 2 Re sum_j c_j exp(2 pi i j theta), j = 1..harmonics <= 8.
 * eaqhm_noise_modulation (kernel: one wave per frame, lanes over the frame's 4 hop samples) analyses e = s - s_recon
 *   (double[L]) on the frames of eaqhm_noise_analyse: c_j = sum_v u[v] exp(-2 pi i j Theta(m hop - 2 hop + v)) / sum_v u[v],
 *   u = (w e)^2, Theta(x) = theta[i] + f0[i] (x - ti0 - i step) / fs at the instant i nearest to x.
 *   theta, f0  double[No_ti]      the fundamental's phase (cycles, [0, 1)) and frequency (Hz) at every instant
 *   voiced     uint8[No_ti]       0: a frame whose nearest instant is this one gets c = 0
 *   mod        double[Nf][2 harmonics]  Re c_1, Im c_1, .. ; zeros where the frame's power is not > 0
 * eaqhm_noise_synth with mod, harmonics, theta, nu applies the gain g_q(n') = sqrt(max(0.01, g^2(theta[q] + nu[q] (n' -
 *   q hop)))) on frame q's samples in the cross-fade, the coefficients (mod, double[Nf][2 harmonics]) blended between
 *   the model's frames at tau[q] as sigma is;
 *   theta, nu  double[Nq]         the output fundamental's phase (cycles) at frame centre q hop and its advance per sample
 *   A mod of zeros gives the plain cross-fade's samples bit for bit.
 * EAQHM_EINVAL for null pointers, L < 1, No_ti < 1, hop outside [1, 1024], harmonics outside [1, 8], step or fs not > 0. */
int eaqhm_noise_modulation(eaqhm_ctx* ctx, const double* e, int64_t L, int32_t hop, const double* theta,
                           const double* f0, const uint8_t* voiced, int32_t No_ti, double ti0, double step, double fs,
                           int32_t harmonics, double* mod);

/* the piecewise-linear formant warp (additions under ABI 6) ----------------------------------
 * A formant warp is a strictly increasing piecewise-linear map W from model frequency to output frequency through
 * (0, 0) and B breakpoints (x_j, y_j), 1 <= B <= 16, continued past the last one with the last slope: a feature at F in
 * the model sits at W(F) in the output.  B = 1 with (x, alpha x) is the formant scale alpha.
 *   f_in       double[B]          x_0 < x_1 < .. , all > 0; shared by all instants / frames
 *   f_out      double[n][B]       y_0 < y_1 < .. , all > 0; one row per instant (n = No_ti) or per noise frame (n = Nf)
 * The kernels evaluate the inverse V = W^-1 at an output frequency q: b = min(#{j : y_j <= q}, B - 1),
 * V(q) = x_{b-1} + (q - y_{b-1}) * ((x_b - x_{b-1}) / (y_b - y_{b-1})) with x_{-1} = y_{-1} = 0, in this order of
 * operations; a row that equals f_in bit for bit is the identity, V(q) = q with no arithmetic.
 * Monotonicity and the range of the slopes are the CALLER'S contract (the Python host checks them): the entry points do
 * not read the device arrays.  A row that breaks the contract gives wrong numbers, never an access out of bounds (the
 * segment scan is bounded by B).
 * eaqhm_modify_amp_warp (kernel: one wave per instant, the envelope nodes of eaqhm_modify_prep in LDS, the wave's row of
 *   the map in LDS) overwrites the amp of an eaqhm_modify_prep that ran with preserve_envelope = 0 and alpha NULL, on the
 *   same stream, with the same beta; eaqhm_modify_synth then runs unchanged:
 *   amp        double[No_ti][Kmax]  A' = exp(E_i(V_i(beta_i f))) for an active slot, 0 for an inactive one and where
 *                                   beta_i f >= fs/2; an instant with an identity row and beta_i == 1 gives |a|, a copy
 * eaqhm_model_envelope_warp: eaqhm_model_envelope with V_i in place of / alpha_i: out[i][t] = E_i(V_i(freqs[t])).
 * eaqhm_noise_warp_map: eaqhm_noise_warp with frame m's spectrum read at w = min(2 pi V_m(t / 2048), pi), t = 0..1024;
 *   f_in, f_out in cycles per sample (Hz / fs).  An identity row returns the frame bit for bit, a silent frame silent.
 * eaqhm_noise_envelope_map: eaqhm_noise_envelope at w = min(2 pi V_m(fnorm[t]), pi).
 * EAQHM_EINVAL for null pointers, B < 1, B > 16 and the limits of the alpha siblings (No_ti < 4, Kmax beyond the LDS
 * budget, F < 1, Nf < 1, order outside [1, 63], fs not finite and > 0).                                              */
int eaqhm_modify_amp_warp(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, double fs,
                          const double* beta, const double* f_in, const double* f_out, int32_t B, double* amp);
int eaqhm_model_envelope_warp(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, const double* f_in,
                              const double* f_out, int32_t B, const double* freqs, int32_t F, double* out);
int eaqhm_noise_warp_map(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf, int32_t order,
                         const double* f_in, const double* f_out, int32_t B, double* sigma_out, double* refl_out);
int eaqhm_noise_envelope_map(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf, int32_t order,
                             const double* f_in, const double* f_out, int32_t B, const double* fnorm, int32_t F,
                             double* out);

/* the discrete-cepstrum spectral envelope (additions under ABI 6) ----------------------------------------
 * A smooth log-amplitude envelope per analysis instant, held as order + 1 coefficients:
 *   C(w) = c_0 + 2 sum_{p=1..order} c_p cos(p w),  w = 2 pi f / fs.
 *   ceps       double[n][order+1]   c_0..c_order per instant / row; a row (-inf, 0, .., 0) is an empty envelope
 * eaqhm_model_cepstrum (kernel: one wave per instant, the nodes, the cosine sums and the Cholesky factor in LDS) fits
 *   instant i to its active slots (am != 0, f > 0; w_n = 2 pi f_n / fs, v_n = ln am_n):
 *   c = argmin sum_n (v_n - C(w_n))^2 + lambda sum_p 8 pi^2 p^2 c_p^2  (c_0 is not penalised).  With lambda > 0 and
 *   at least one node the system is positive definite, so an instant with fewer nodes than coefficients is solved like
 *   any other.  An instant without nodes gives (-inf, 0, .., 0); a pivot that is not finite or not > 0 gives a NaN row.
 * eaqhm_modify_amp_cepstrum (one wave per instant) overwrites the amp of an eaqhm_modify_prep that ran with
 *   preserve_envelope = 0 and alpha NULL, on the same stream, with the same beta; eaqhm_modify_synth then runs unchanged:
 *   amp        double[No_ti][Kmax]  A' = exp(C_i(read_i(beta_i f))) for an active slot, 0 for an inactive one and where
 *                                   beta_i f >= fs/2.  There is no unit rule: at beta = 1 the amplitudes are C's too.
 *   read_i(q) is q (alpha NULL, no warp group), q / alpha_i (alpha double[No_ti]) or V_i(q), the inverse of the formant
 *   warp above (f_in double[B], f_out double[No_ti][B]); C is read at min(max(read_i(q), 0), fs/2): held past Nyquist.
 * eaqhm_cepstrum_envelope (one wave per row): out[i][t] = C_i(read_i(freqs[t])), natural-log amplitude, not muted;
 *   -inf on an empty row.  alpha is double[n], f_out double[n][B].
 * The readout is Clenshaw's recurrence from one cos; c_0 is added last.  The entry points do not read the device arrays:
 * finite coefficients and a monotone map are the CALLER'S contract (the Python host checks them).
 * EAQHM_EINVAL for null pointers (alpha and the warp group are optional: NULL, and NULL, NULL, 0), order outside [1, 63],
 * lambda not finite or not > 0, alpha and the warp group both given, the warp group given in part or B outside [1, 16],
 * No_ti < 1 (< 4 for eaqhm_modify_amp_cepstrum, as for its siblings), n < 1, F < 1, fs not finite and > 0, Kmax beyond
 * the LDS budget of the fit (4 waves x (2 Kmax + 2 order + 2 + (order + 1) ((order + 1) | 1)) doubles <= 160 KiB).   */
int eaqhm_model_cepstrum(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, double fs, int32_t order,
                         double lambda, double* ceps);
int eaqhm_modify_amp_cepstrum(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, double fs,
                              const double* beta, const double* ceps, int32_t order, const double* alpha,
                              const double* f_in, const double* f_out, int32_t B, double* amp);
int eaqhm_cepstrum_envelope(eaqhm_ctx* ctx, const double* ceps, int32_t n, int32_t order, double fs,
                            const double* alpha, const double* f_in, const double* f_out, int32_t B,
                            const double* freqs, int32_t F, double* out);

/* time alignment of two models: banded DTW over cepstral rows (additions under ABI 6) ------------------
 * The table has nA x nB cells, cell (i, j) pairing row i of A with row j of B.  THE BAND: half-width r rows of B around
 * the scaled diagonal, centre c_i = (2 i (nB-1) + (nA-1)) / (2 (nA-1)) in 64-bit integer division (c_0 = 0 when nA = 1);
 * cell (i, j) is in the band iff |j - c_i| <= r and 0 <= j < nB.
 *   band       double[nA][W], W = 2 r + 1   cell (i, j) at [i][j - c_i + r]; cells outside the table hold +inf
 *   ptr        uint8[nA][W]                 back-pointer per cell, same layout: 0 from (i-1, j-1), 1 from (i-1, j),
 *                                           2 from (i, j-1), 3 the start (0, 0); written only inside the table
 *   path       int32[(nA + nB - 1)][2]      8-byte aligned; on return the first *path_len pairs (i, j), from (0, 0) to
 *                                           (nA-1, nB-1)
 *   path_len   int32[1], total double[1]    device memory: the path's length (-1: the walk failed), D(nA-1, nB-1)
 * r must admit a path: r >= nB - 1 when nA = 1, else r >= ceil((nB - 1) / (nA - 1)); r = max(nA, nB) - 1 is the full
 * table.
 * eaqhm_cepstrum_cost fills the whole band with the local cost between cepsA double[nA][order+1] and cepsB
 *   double[nB][order+1] (the layout of eaqhm_model_cepstrum), dC = cepsA[i] - cepsB[j]:
 *   d(i, j) = c0_weight dC_0^2 + 2 sum_{p=1..order} dC_p^2  (at c0_weight = 1 the mean over frequency of the squared
 *   difference of the two log envelopes, neper^2), the differences formed directly; a row whose c_0 is -inf is empty:
 *   d = 0 between two empty rows, empty_cost between an empty row and another.  Cells outside the table get +inf.
 *   (Kernel: a block keeps 16 rows of A in LDS and streams the B rows of its band through LDS, 64 at a time.)
 * eaqhm_dtw runs on any band of finite costs >= 0 (+inf outside the table), in place: band holds d on entry and
 *   D(0,0) = d(0,0), D(i,j) = d(i,j) + min(D(i-1,j-1), D(i-1,j), D(i,j-1)) on return, predecessors outside the table or
 *   the band counting +inf; on equal values the lower code wins (a candidate replaces the current one only when strictly
 *   smaller), so D, ptr and the path are fully determined.  Forward pass: one wave per 64 x 64 tile of the table, one
 *   launch per tile anti-diagonal on the context's stream (ceil(nA/64) + ceil(nB/64) - 1 at most; only the tiles that
 *   meet the band are launched); the order between dependent tiles is stream order, no workgroup waits on another.
 *   Then one launch walks the back-pointers (a single lane, at most nA + nB - 1 steps).
 * The entry points do not read the device arrays: finite costs >= 0 and (-inf, 0, .., 0) as the only non-finite rows
 * are the CALLER'S contract (the Python host checks them).
 * EAQHM_EINVAL for null pointers, order outside [1, 63], c0_weight or empty_cost not finite or < 0, nA or nB outside
 * [1, 2^30], r < 0, r >= 2^30, or r too small to admit a path.                                                       */
int eaqhm_cepstrum_cost(eaqhm_ctx* ctx, const double* cepsA, int32_t nA, const double* cepsB, int32_t nB, int32_t order,
                        double c0_weight, double empty_cost, int32_t r, double* band_out);
int eaqhm_dtw(eaqhm_ctx* ctx, double* band, int32_t nA, int32_t nB, int32_t r, uint8_t* ptr, int32_t* path,
              int32_t* path_len, double* total);

/* a harmonic model from f0 and cepstral rows (additions under ABI 6) -----------------------------------
 * eaqhm_model_build (kernel: one wave per instant, four per block, the row's coefficients in the wave's LDS, lanes over
 *   the harmonics in chunks of 64) writes the records double[n][3 Kmax + 1] (|a| | f | phase | a0, the layout above) of
 *   the model whose slot k holds harmonic h = k + 1 of f0:
 *   f0         double[n]            Hz; read at voiced instants only
 *   theta      double[n]            the fundamental's phase in cycles at the instant (the host's recurrence, §9.7)
 *   voiced     uint8[n]             0: every slot of the instant is inactive
 *   ceps       double[n][order+1]   the envelope, the layout of eaqhm_model_cepstrum; a row (-inf, 0, .., 0) is empty
 *   a0         double[n]            copied to the records' last column
 *   Slot k of instant i is active iff voiced[i], the row is not empty, k < Kcap, and h f0_i < fs/2 (the float64 product
 *   against 0.5 fs, as the host forms it); then f = h f0_i, |a| = exp(C_i(f)) (Clenshaw from one cosine, c_0 added last,
 *   as eaqhm_cepstrum_envelope reads it) and phase = wrap(2 pi frac(h theta_i) + Phi_i(f)) in (-pi, pi], with
 *   Phi_i(f) = -2 sum_p c_p sin(2 pi p f / fs), the minimum-phase response of the envelope, from the same recurrence
 *   (cosine sum b_1 cos t - b_2, sine sum b_1 sin t); zero_phase = 1 sets Phi = 0.  A cell whose exp underflows to 0 is
 *   inactive.  Inactive cells are written as exact zeros in all three fields: the records need no memset.
 * eaqhm_cepstrum_phase is eaqhm_cepstrum_envelope with Phi in place of C: out[i][t] = Phi_i(read_i(freqs[t])) in
 *   radians, as the series gives it (not wrapped); 0 on an empty row.  The same grid and optional alpha / warp group.
 * The entry points do not read the device arrays: finite f0 in (0, fs/2) at voiced instants, finite theta and
 * coefficients are the CALLER'S contract (the Python host checks them).
 * EAQHM_EINVAL for null pointers, n < 2 (n < 1 for eaqhm_cepstrum_phase), order outside [1, 63], fs not finite and > 0,
 * Kcap outside [1, 1706], Kmax outside [1, Kcap], zero_phase not 0 or 1, and eaqhm_cepstrum_envelope's rules.         */
int eaqhm_model_build(eaqhm_ctx* ctx, const double* f0, const double* theta, const uint8_t* voiced, const double* ceps,
                      int32_t order, const double* a0, int32_t n, double fs, int32_t Kmax, int32_t Kcap,
                      int32_t zero_phase, double* records);
int eaqhm_cepstrum_phase(eaqhm_ctx* ctx, const double* ceps, int32_t n, int32_t order, double fs, const double* alpha,
                         const double* f_in, const double* f_out, int32_t B, const double* freqs, int32_t F,
                         double* out);

/* the noise model to and from cepstral rows (additions under ABI 6) ----------------------------------
 * A frame (sigma, k_1..k_order) has the log-amplitude spectrum C(w) = ln(sigma / |A(e^{jw})|) = c_0 + 2 sum_q c_q
 * cos(q w), the layout of eaqhm_model_cepstrum.  The level is that of a spectral density per sample (sigma is the
 * standard deviation of the excitation), not the level of the harmonic envelope.
 * eaqhm_noise_cepstrum (kernel: one wave per frame, four per block; A(z) by the step-up into the wave's LDS, then
 *   ceps_order steps of the LPC-to-cepstrum recursion, lanes over the terms of a step, one cross-lane sum per step):
 *   ceps       double[Nf][ceps_order+1]  c_0 = ln sigma, c_q = h_q / 2, h_n = -a_n - (sum_{k=1..n-1} (k h_k) a_{n-k}) / n
 *                                        with a_j = 0 for j > order: the exact cepstrum of the frame, cut at ceps_order;
 *                                        a silent frame (sigma == 0) gives (-inf, 0, .., 0)
 * eaqhm_noise_from_cepstrum (kernel: one wave per row, eight per block, the block shape of eaqhm_noise_warp: the cosine
 *   table shared by the block, P[0..1024] and the row in the wave's LDS, 77 968 bytes) fits a frame of `order` to each
 *   row: P[t] = exp(2 (C(w_t) - c_0)) on the grid w_t = pi t / 1024 by Clenshaw's recurrence, the autocorrelation and
 *   the Levinson-Durbin recursion of eaqhm_noise_warp, sigma_out = exp(c_0) sqrt(E).  c_0 does not enter P, so refl_out
 *   does not depend on it.  A row (-inf, 0, .., 0) gives sigma_out = 0 and zeros.
 *   sigma_out  double[Nf], refl_out double[Nf][order]
 * The entry points do not read the device arrays: |k| < 1, finite coefficients and 4 sum_q |c_q| <= 600 (exp stays in
 * the normal range) are the CALLER'S contract (the Python host checks them).
 * EAQHM_EINVAL for null pointers, Nf < 1, order or ceps_order outside [1, 63].                                        */
int eaqhm_noise_cepstrum(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf, int32_t order,
                         int32_t ceps_order, double* ceps);
int eaqhm_noise_from_cepstrum(eaqhm_ctx* ctx, const double* ceps, int32_t Nf, int32_t ceps_order, int32_t order,
                              double* sigma_out, double* refl_out);

/* the joint-density Gaussian mixture of the spectral conversion (additions under ABI 6) ------------------
 * Rows Z double[N][D] are the CENTRED joint vectors c_n = [x_n | y_n] - zbar; the mixture has M components.
 * 1 <= N <= 2^36, 1 <= D <= 128 (1 <= dx, dy <= 64 for the regression), 1 <= M <= 64; any value in range, none needs to
 * be a multiple of 4 or 16: the kernels pad in LDS.  All three contract on the matrix pipe (v_mfma_f64_16x16x4_f64).
 * eaqhm_gmm_estep (kernel: 64 rows per block, four waves of one 16-row tile; W_m in 16-row panels through LDS, each
 *   contracted over its lower-triangle columns only; squared norms, the log-sum-exp over m and gamma in the same launch):
 *   mu         double[M][D]      centred means
 *   W          double[M][D][D]   W_m = L_m^-1, lower triangular, L_m L_m^T = Sigma_m; entries above the diagonal are not read
 *   k          double[M]         k_m = ln w_m - (D ln 2 pi + 2 sum_i ln L_m[i][i]) / 2
 *   gamma_out  double[N][M]      with q_nm = ||W_m (c_n - mu_m)||^2, lp_nm = k_m - q_nm / 2, max_n = max_m lp_nm,
 *                                e_nm = exp(lp_nm - max_n), s_n = sum_m e_nm (m ascending): gamma_nm = e_nm / s_n
 *   ll_out     double[N]         ll_n = max_n + ln s_n.  A row so far from every mean that each q_nm overflows to +inf
 *                                (max_n = -inf) gets ll_n = -inf and gamma_nm = 1 / M instead of NaN.
 *   The marginal E-step of the conversion is this entry point with D = dx.
 * eaqhm_gmm_mstep (kernels: one block per (row chunk, component): the weighted Gramian of [c | 1] over the lower-triangle
 *   16 x 16 tiles, A operand gamma c, B operand c, S1 and S0 in the row of the ones; then one thread per entry adds the
 *   chunks in index order): S0[m] = sum_n gamma_nm, S1[m][i] = sum_n gamma_nm c_ni, S2[m][i][j] = sum_n gamma_nm c_ni c_nj.
 *   S0 double[M], S1 double[M][D], S2 double[M][D][D], the upper triangle of S2_m a copy of the lower.
 *   Rows are cut into chunks of R = max(512, 64 ceil(ceil(N / 128) / 64)) rows, a function of N alone: no atomics, no
 *   dependence on the device or on timing, the same bits on every run.
 *   work       double[eaqhm_gmm_work_len]  ceil(N / R) M T 256 words, T = nt (nt + 1) / 2, nt = ceil((D + 1) / 16):
 *                                the chunks' tiles; 755 MB at N = 10^6, M = 64, D = 128.  eaqhm_gmm_work_len returns -1
 *                                for sizes out of range.
 * eaqhm_gmm_regress (kernel: 64 rows per block; x_n A_m^T on the matrix pipe in panels of 16 columns of y, then
 *   y_n += gamma_nm (A_m x_n + b_m), m ascending):
 *   X double[N][dx], gamma double[N][M], A double[M][dy][dx], b double[M][dy], Y_out double[N][dy]
 * The entry points do not read the device arrays: finite values are the CALLER'S contract (the Python host checks them).
 * EAQHM_EINVAL for null pointers and sizes outside the ranges above.                                                  */
int64_t eaqhm_gmm_work_len(int64_t N, int32_t D, int32_t M);
int eaqhm_gmm_estep(eaqhm_ctx* ctx, const double* Z, int64_t N, int32_t D, int32_t M, const double* mu, const double* W,
                    const double* k, double* gamma_out, double* ll_out);
int eaqhm_gmm_mstep(eaqhm_ctx* ctx, const double* Z, const double* gamma, int64_t N, int32_t D, int32_t M, double* work,
                    double* S0, double* S1, double* S2);
int eaqhm_gmm_regress(eaqhm_ctx* ctx, const double* X, const double* gamma, const double* A, const double* b, int64_t N,
                      int32_t dx, int32_t dy, int32_t M, double* Y_out);

/* delta rows and the maximum-likelihood trajectory of the conversion (additions under ABI 6): the
 * declarations are in eaqhm_mlpg.h, which this header includes.                                                      */
#include "eaqhm_mlpg.h"
/* the global-variance ascent from that trajectory (additions under ABI 6): declared in eaqhm_gv.h.     */
#include "eaqhm_gv.h"
/* the discrete cepstrum on an all-pass warped axis (additions under ABI 6): declared in eaqhm_cepwarp.h. */
#include "eaqhm_cepwarp.h"
/* the k-means codebook that starts the mixture (additions under ABI 6): declared in eaqhm_kmeans.h.    */
#include "eaqhm_kmeans.h"
/* the conditional E-step of the trajectory refinement (additions under ABI 6): declared in eaqhm_mlpg_em.h. */
#include "eaqhm_mlpg_em.h"
/* nearest rows, the search of the non-parallel training (additions under ABI 6): declared in eaqhm_nn.h. */
#include "eaqhm_nn.h"
/* the SWIPE' pitch estimator's loudness, scores and pick stages (additions under ABI 6): declared in eaqhm_swipe.h. */
#include "eaqhm_swipe.h"
/* the continuous pitch track: Viterbi forward pass, backtrack and refinement (additions under ABI 6): declared in eaqhm_viterbi.h. */
#include "eaqhm_viterbi.h"
/* formant tracks: the poles of the all-pole envelope, the candidates and their Viterbi decode (additions under ABI 6): declared in eaqhm_formant.h. */
#include "eaqhm_formant.h"
/* transient onsets: log band energies, their flux and the peak rule (additions under ABI 6): declared in eaqhm_onset.h. */
#include "eaqhm_onset.h"

#ifdef __cplusplus
}
#endif
#endif
