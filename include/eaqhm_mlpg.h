/* eaqhm_mlpg.h — part of the C ABI of libeaqhm_hip.so (included by eaqhm_hip.h, which declares eaqhm_ctx and the
 * error codes): delta rows of cepstral rows and the trajectory solve of the spectral conversion.                      */
#ifndef EAQHM_MLPG_H
#define EAQHM_MLPG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* delta rows and the maximum-likelihood trajectory of the conversion (additions under ABI 6) ----------
 * A run is a maximal stretch of consecutive non-empty rows; an empty row has -inf in column 0.  span = L in [1, 8]; the
 * window is w_tau = tau / (2 sum_k k^2), k = 1 .. L.
 * eaqhm_ceps_delta (kernel: one thread per entry): out[t][j] = sum_tau w_tau (C[clip(t + tau)][j] - C[clip(t - tau)][j]),
 *   tau ascending, clip holding the index inside the row's own run, whose edges are found from column 0 of at most span
 *   neighbours on each side.  An empty row gets a row of zeros.
 *   C double[n][cols], out double[n][cols]; 1 <= n <= 2^31, 1 <= cols <= 128.
 * eaqhm_mlpg_solve (kernels: one thread per (row, column) forms row i of the band of R and q_i in `work`; then one lane
 *   per system (run, column) factorises R = L D L^T (the root-free banded Cholesky, half-bandwidth min(2 span, T - 1)) and
 *   substitutes forward in one sweep over the run and backward in a second; the last rows of L in LDS, all of L in `work`):
 *   for every run and every column d < dy, with W the T x T matrix of the delta rule on the run,
 *     R = diag(P^s) + W^T diag(P^D) W,   q = r^s + W^T r^D,   R y = q.
 *   P, r       double[n][2 dy]   precisions and precision-weighted means, the static half [0, dy) first, the delta half after
 *   run_start, run_len  int64[n_runs]  the runs, disjoint and ascending, inside [0, n): the CALLER'S contract (a run whose
 *                                bounds leave [0, n) is skipped)
 *   work       double[eaqhm_mlpg_work_len]  n (2 span + 2) dy words; eaqhm_mlpg_work_len returns -1 for sizes out of range
 *   Y          double[n][dy]     rows outside every run are not written
 *   P^s > 0 and P^D >= 0 make R positive definite; the entry point does not read the device arrays.  With P^D = 0 the
 *   result is r^s / P^s, one rounding.  No atomics, fixed order of every sum: the same bits on every run.
 * EAQHM_EINVAL, nothing launched, for null pointers, n < 1, dy outside [1, 64], cols outside [1, 128], span outside
 * [1, 8], n_runs < 0 or > n, run_start or run_len null while n_runs > 0.  n_runs = 0 is valid and does nothing.        */
int eaqhm_ceps_delta(eaqhm_ctx* ctx, const double* C, int64_t n, int32_t cols, int32_t span, double* out);
int64_t eaqhm_mlpg_work_len(int64_t n, int32_t dy, int32_t span);
int eaqhm_mlpg_solve(eaqhm_ctx* ctx, const double* P, const double* r, int64_t n, int32_t dy, int32_t span,
                     const int64_t* run_start, const int64_t* run_len, int64_t n_runs, double* work, double* Y);

#ifdef __cplusplus
}
#endif
#endif
