/* eaqhm_formant.h — part of the C ABI of libeaqhm_hip.so (included by eaqhm_hip.h, which declares eaqhm_ctx and the error
 * codes): formant tracks.  The poles of every frame's all-pole envelope by the Aberth-Ehrlich iteration,
 * the formant candidates among them, and a Viterbi decode that sorts the candidates into F1..FN over time.  No atomics,
 * every word has one writer, every sum has a fixed order.  The entry points allocate nothing and do not read the device
 * arrays: |k| < 1 and finite tables are the CALLER'S contract (the Python host checks them).                            */
#ifndef EAQHM_FORMANT_H
#define EAQHM_FORMANT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define EAQHM_FORMANT_ORDER 63     /* p at most: lane k of a wave owns root k */
#define EAQHM_FORMANT_ITMAX 64     /* Aberth steps at most; iters = ITMAX + 1 marks a frame that did not finish */
#define EAQHM_FORMANT_CAND 8       /* KC: candidates kept per frame, the lowest in frequency */
#define EAQHM_FORMANT_TRACKS 4     /* N at most */
#define EAQHM_FORMANT_STATES 495   /* C(8 + 4, 4): states at most */

/* DESIGN.md §14.1 — the poles of every frame (additions under ABI 6).
 * eaqhm_allpole_roots: one wave per frame.  a_0..a_p by the model's step-up of the frame's reflection coefficients
 *   (a_0 = 1), P(z) = z^p + a_1 z^(p-1) + .. + a_p.  pe = the largest i with k_i != 0 (0: none); the last p - pe places
 *   of the frame are the exact roots (0, 0), the iteration runs on degree pe.  Start z_k = r0 exp(i (2 pi k / pe +
 *   pi / (2 pe))), r0 = exp(log|a_pe| / pe).  Per step, per lane k < pe not yet accepted: one Horner pass in ascending j
 *   gives P(z_k), P'(z_k) and s_k = sum_j |a_j| |z_k|^(pe-j); the lane is accepted, and frozen, once
 *   |P(z_k)| <= 8 pe 2^-53 s_k; otherwise N = P / P', S = sum_{j != k, ascending j} 1 / (z_k - z_j) over the OLD iterate
 *   (frozen lanes included), z_k -= N / (1 - N S).  The frame ends when every lane is accepted or after ITMAX steps.
 *   refl   double[Nf][p]      1 <= p <= 63, 1 <= Nf < 2^31, |k| < 1
 *   roots  double[Nf][p][2]   (re, im)
 *   iters  int32[Nf]          the steps taken, 0 .. ITMAX; ITMAX + 1: not finished (the last iterate is written)         */
int eaqhm_allpole_roots(eaqhm_ctx* ctx, const double* refl, int64_t Nf, int32_t p, double* roots, int32_t* iters);

/* DESIGN.md §14.2 — the formant candidates of every frame (additions under ABI 6).
 * eaqhm_formant_candidates: one wave per frame.  A pole qualifies with im > 0, f = atan2(im, re) fs / (2 pi) in
 *   [fmin, fmax] and bw = -log(sqrt(re^2 + im^2)) fs / pi <= bw_max; the qualifying poles in ascending f (equal f: the
 *   lower root index first), the lowest EAQHM_FORMANT_CAND kept.  A frame with iters = ITMAX + 1 has none.
 *   roots, iters  as above;  fs > 0, fmin, fmax, bw_max finite
 *   cand_f, cand_b  double[Nf][8]   NaN beyond the count
 *   count           int32[Nf]                                                                                         */
int eaqhm_formant_candidates(eaqhm_ctx* ctx, const double* roots, const int32_t* iters, int64_t Nf, int32_t p, double fs,
                             double fmin, double fmax, double bw_max, double* cand_f, double* cand_b, int32_t* count);

/* DESIGN.md §14.3 — the tracker (additions under ABI 6).
 * A state gives each of the N slots a candidate index in [0, 8) or -1, "absent", the used indices strictly increasing
 * along the slots: S = C(8 + N, N) states (9, 45, 165, 495), the table in lexicographic order of the tuples.  A state
 * that uses an index >= count[t] has local cost +inf at t.
 *   local(s, t) = sum_n (s_n >= 0 ? L[t][n][s_n] : absent_cost)                   slot order, from 0.0
 *   J[a][b]     = w_jump |lf[t][b] - lf[t-1][a]|, a < count[t-1], b < count[t]; 0 where either side is absent
 *   D[s', 0]    = local(s', 0)
 *   D[s', t]    = min_s (D[s, t-1] + sum_n J[s_n][s'_n]) + local(s', t)          the first minimum in state order
 * eaqhm_formant_forward: one block of 512 threads walks the T steps, thread s' scans the predecessors.
 *   L       double[T][N][8], lf double[T][8]   finite everywhere (entries beyond the count are not looked at)
 *   count   int32[T]            values outside [0, 8] are clamped
 *   states  int8[S][N]          the table above
 *   1 <= N <= 4, 1 <= T < 2^31; w_jump and absent_cost finite and >= 0
 *   bp      int16[T][S]         the predecessor of every state at every step; row 0 holds the state itself
 *   last    double[S]           D[., T-1]
 * eaqhm_formant_backtrack: one wave finds the first minimum of last, one lane walks bp.
 *   q       int32[T]            the state at every frame, in [0, S)
 *   total   double[1]           the path's cost
 * EAQHM_EINVAL, nothing launched, no output touched, for null pointers and values outside the ranges above.            */
int eaqhm_formant_forward(eaqhm_ctx* ctx, const double* L, const double* lf, const int32_t* count, const int8_t* states,
                          int32_t N, int64_t T, double w_jump, double absent_cost, int16_t* bp, double* last);
int eaqhm_formant_backtrack(eaqhm_ctx* ctx, const int16_t* bp, const double* last, int32_t N, int64_t T, int32_t* q,
                            double* total);

#ifdef __cplusplus
}
#endif
#endif
