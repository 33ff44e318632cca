/* eaqhm_cepwarp.h — part of the C ABI of libeaqhm_hip.so (included by eaqhm_hip.h, which declares eaqhm_ctx and the
 * error codes): the discrete cepstrum on an all-pass warped frequency axis.                                            */
#ifndef EAQHM_CEPWARP_H
#define EAQHM_CEPWARP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the warped discrete cepstrum (additions under ABI 6) -------------------------------------------------
 * For a coefficient a = cep_warp, |a| <= 0.9, the all-pass warp of w = 2 pi f / fs is
 *     Omega_a(w) = w + 2 atan2(a sin w, 1 - a cos w),
 * strictly increasing on [0, pi] with Omega_a(0) = 0, Omega_a(pi) = pi; a > 0 stretches the low band.  A warped row
 * c_0..c_P describes C(w) = c_0 + 2 sum_p c_p cos(p Omega_a(w)) and the minimum-phase response
 * Phi(w) = -2 sum_p c_p sin(p Omega_a(w)).  The rows keep eaqhm_model_cepstrum's layout; nothing in a row says which
 * axis it is on: passing the a of the fit to every readout is the CALLER'S contract.
 * Each entry point is its sibling of eaqhm_hip.h with one more argument, `double cep_warp`, last: the same arrays, the
 * same ranges, the same launch shape and LDS, the same rules for empty rows, the hold outside [0, fs/2] and the read
 * frequency (q, q / alpha or W^-1(q), formed in Hz before the warp, so the formant controls keep acting in Hz).
 *   eaqhm_model_cepstrum_warped        the fit with the nodes at Omega_a(w_n) (one atan2 per node, as they are staged);
 *                                      the penalty lambda sum 8 pi^2 p^2 c_p^2 is smoothness on the warped axis
 *   eaqhm_modify_amp_cepstrum_warped   A' = exp(C(read)) off a warped row
 *   eaqhm_cepstrum_envelope_warped     C on a frequency grid
 *   eaqhm_cepstrum_phase_warped        Phi on a frequency grid
 *   eaqhm_model_build_warped           the records of a harmonic model from f0 and warped rows
 *   eaqhm_noise_from_cepstrum_warped   a noise frame from a warped row: P[t] = exp(4 sum_q c_q cos(q Omega_a(w_t)))
 * The readouts take cos and sin of Omega_a(w) from those of w / 2 by the rational map
 *     u = (1 + a) sin(w/2), v = (1 - a) cos(w/2):  cos Omega = (v - u)(v + u) / (u^2 + v^2),  sin Omega = 2 u v / (u^2 + v^2)
 * (tan(Omega / 2) = ((1 + a) / (1 - a)) tan(w / 2)): one division per cell, no atan2, and no cancellation in the
 * denominator, which is at least (1 - |a|)^2.  cep_warp = 0 describes the linear axis, but not in the sibling's bits.
 * EAQHM_EINVAL, nothing launched, for the sibling's reasons and unless cep_warp is finite and |cep_warp| <= 0.9.      */
int eaqhm_model_cepstrum_warped(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, double fs,
                                int32_t order, double lambda, double* ceps, double cep_warp);
int eaqhm_modify_amp_cepstrum_warped(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, double fs,
                                     const double* beta, const double* ceps, int32_t order, const double* alpha,
                                     const double* f_in, const double* f_out, int32_t B, double* amp, double cep_warp);
int eaqhm_cepstrum_envelope_warped(eaqhm_ctx* ctx, const double* ceps, int32_t n, int32_t order, double fs,
                                   const double* alpha, const double* f_in, const double* f_out, int32_t B,
                                   const double* freqs, int32_t F, double* out, double cep_warp);
int eaqhm_cepstrum_phase_warped(eaqhm_ctx* ctx, const double* ceps, int32_t n, int32_t order, double fs,
                                const double* alpha, const double* f_in, const double* f_out, int32_t B,
                                const double* freqs, int32_t F, double* out, double cep_warp);
int eaqhm_model_build_warped(eaqhm_ctx* ctx, const double* f0, const double* theta, const uint8_t* voiced,
                             const double* ceps, int32_t order, const double* a0, int32_t n, double fs, int32_t Kmax,
                             int32_t Kcap, int32_t zero_phase, double* records, double cep_warp);
int eaqhm_noise_from_cepstrum_warped(eaqhm_ctx* ctx, const double* ceps, int32_t Nf, int32_t ceps_order, int32_t order,
                                     double* sigma_out, double* refl_out, double cep_warp);

#ifdef __cplusplus
}
#endif
#endif
