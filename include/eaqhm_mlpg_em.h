/* eaqhm_mlpg_em.h — part of the C ABI of libeaqhm_hip.so (included by eaqhm_hip.h, which declares eaqhm_ctx and the
 * error codes): the conditional E-step of the EM refinement of the trajectory conversion.                             */
#ifndef EAQHM_MLPG_EM_H
#define EAQHM_MLPG_EM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the posteriors of the mixture's components given the source rows and a trajectory (additions under ABI 6; DESIGN.md
 * §12.4; Toda, Black & Tokuda 2007) ------------------------------------------------------------------------------------
 * eaqhm_mlpg_estep (one kernel, 64 rows per block, FP64 MFMA): for every row t of every run and every component m,
 *     Yd_t = [y_t | (W y)_t]                     W the run's delta rule (eaqhm_ceps_delta's: tau ascending, the index
 *                                                clipped to the row's own run), formed in the kernel from Y
 *     q_tm = sum_j py_mj (Yd_tj - (sum_k A_mjk X_tk + bq_mj))^2,       j over the 2 dy columns
 *     lp_tm = ln prior_tm + kc_m - q_tm / 2
 *     ll_t = ln sum_m exp lp_tm (about the largest lp),   gamma_tm = exp(lp_tm - ll_t)
 *   X          double[n][dx]        centred dynamic source rows
 *   prior      double[n][M]         p(m | X_t): the marginal E-step's gamma
 *   A          double[M][2 dy][dx]  regression matrices, the static half of the target first, the delta half after
 *   bq         double[M][2 dy]      b_m + ybar
 *   py         double[M][2 dy]      reciprocal conditional variances
 *   kc         double[M]            (1/2) sum_j ln py_mj - dy ln 2 pi
 *   Y          double[n][dy]        the static trajectory; dy counts the STATIC target columns, as in eaqhm_mlpg_solve
 *   run_start, run_len  int64[n_runs]  the runs, disjoint and ascending, inside [0, n): the CALLER'S contract (a run whose
 *                                   bounds leave [0, n) is skipped)
 *   gamma_out  double[n][M], ll_out double[n]   rows outside every run are not written
 *   A component whose prior is 0 on a row is left out of that row: its gamma is exactly 0 and it does not enter the
 *   maximum.  A row on which every remaining lp is -inf (a quadratic form overflowed) gets ll = -inf and gamma = its prior
 *   row.  No work buffer.  No atomics, one writer per word, fixed order of every sum; a row's results depend on that row,
 *   its run neighbours and the parameters only: the same bits on every launch and wherever the run lies in the array.
 * EAQHM_EINVAL, nothing launched, for null pointers, n < 1 or > 2^31, dx outside [1, 64], dy outside [1, 32], M outside
 * [1, 64], span outside [1, 8], n_runs < 0 or > n, run_start or run_len null while n_runs > 0.  n_runs = 0 is valid and
 * does nothing.                                                                                                       */
int eaqhm_mlpg_estep(eaqhm_ctx* ctx, const double* X, const double* prior, const double* A, const double* bq,
                     const double* py, const double* kc, const double* Y, int64_t n, int32_t dx, int32_t dy, int32_t M,
                     int32_t span, const int64_t* run_start, const int64_t* run_len, int64_t n_runs, double* gamma_out,
                     double* ll_out);

#ifdef __cplusplus
}
#endif
#endif
