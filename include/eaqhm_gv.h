/* eaqhm_gv.h — part of the C ABI of libeaqhm_hip.so (included by eaqhm_hip.h, which declares eaqhm_ctx and the
 * error codes): the global-variance term of the trajectory conversion.                                                */
#ifndef EAQHM_GV_H
#define EAQHM_GV_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the global-variance ascent from the maximum-likelihood trajectory (additions under ABI 6) -----------
 * P, r, the runs and the ranges of n, dy and span are eaqhm_mlpg_solve's contract (eaqhm_mlpg.h): R and q are its
 * system, block-diagonal over the runs.  N is the number of rows in runs, omega = 1 / (2 N), and per column d < dy
 *     m = (1/N) sum_t y_t,  v = (1/N) sum_t (y_t - m)^2,
 *     L_d(y) = -(omega / 2)(y^T R y - 2 q^T y) - (1/2) gv_prec[d] (v - gv_mean[d])^2.
 * eaqhm_gv_ascend: Y holds y_ML on entry.  Start: y <- m + sqrt(gv_mean[d] / v)(y - m).  Then `iters` times, every row
 * from the old y (a Jacobi sweep), span = L:
 *     g_t = omega (q - R y)_t - gv_prec[d] (v - gv_mean[d]) (2 / N) (y_t - m)
 *     h_t = (4 L + 1) omega R_tt + gv_prec[d] (2 / N) (|v - gv_mean[d]| + 2 v)
 *     y_t <- y_t + g_t / h_t.
 * A column with N < 2 or v(y_ML) = 0 is frozen: Y keeps its bits.  trace[k][d] = L_d(y^(k)), k = 0 .. iters; every
 * entry of a frozen column is L_d(y_ML).
 *   (kernels: one thread per (row, column) forms the band of R and q in `work`; then two launches per sweep over chunks
 *   of eaqhm_gv_chunk_rows(n) rows, one block a chunk: the first writes per (chunk, column) the sums of (y - m)^2, y (R y)
 *   and q y, the second re-adds them, writes trace[k], steps into a second buffer and writes the new per-chunk sums of y;
 *   a closing launch writes trace[iters] and copies the result into Y when it sits in the second buffer; 2 iters + 6
 *   launches with a trace, 2 iters + 4 or 5 without.  Order between launches is stream order alone; no
 *   atomics; every sum in a fixed order, a fixed tree within a chunk and ascending across chunks: the same bits on
 *   every run.)
 *   gv_mean, gv_prec  double[dy]  the target's mean of v and the precision of v with the caller's weight folded in;
 *                                 both > 0 and finite: the CALLER'S contract
 *   iters      0 .. 10000; 0 returns the start
 *   work       double[eaqhm_gv_work_len]; eaqhm_gv_work_len returns -1 for sizes out of range
 *   Y          double[n][dy]     in: y_ML, out: the result; rows outside every run are neither read nor written
 *   trace      double[iters + 1][dy], or null
 * eaqhm_gv_chunk_rows: max(64, 64 ceil(ceil(n / 512) / 64)), a function of n alone; -1 for n outside [1, 2^31].
 * EAQHM_EINVAL, nothing launched, for null pointers (trace excepted), n < 1, dy outside [1, 64], span outside [1, 8],
 * n_runs < 0 or > n, run_start or run_len null while n_runs > 0, iters outside [0, 10000].  n_runs = 0 is valid and does
 * nothing.  The entry point does not read the device arrays.                                                           */
int64_t eaqhm_gv_chunk_rows(int64_t n);
int64_t eaqhm_gv_work_len(int64_t n, int32_t dy, int32_t span);
int eaqhm_gv_ascend(eaqhm_ctx* ctx, const double* P, const double* r, int64_t n, int32_t dy, int32_t span,
                    const int64_t* run_start, const int64_t* run_len, int64_t n_runs, const double* gv_mean,
                    const double* gv_prec, int32_t iters, double* work, double* Y, double* trace);

#ifdef __cplusplus
}
#endif
#endif
