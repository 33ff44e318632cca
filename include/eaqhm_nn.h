/* eaqhm_nn.h — part of the C ABI of libeaqhm_hip.so (included by eaqhm_hip.h, which declares eaqhm_ctx and the error
 * codes): for every row of one set, the nearest row of another, the search behind the training of a conversion from
 * speech that is not parallel.                                                                      */
#ifndef EAQHM_NN_H
#define EAQHM_NN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* nearest rows (additions under ABI 6) ---------------------------------------------------------------
 * A double[nA][lda], B double[nB][ldb]: the first D columns of a row are used, the others are never read.
 * 1 <= nA, nB < 2^31, 1 <= D <= 128, D <= lda, D <= ldb; none needs to be a multiple of 4, 16 or 64: the kernels pad in
 * LDS with zeros.
 * eaqhm_nn_rows (three kernels on the context's stream, ordered by the stream alone; no atomics, every word has one
 *   writer: the same bits on every run, every device and any split count):
 *   1. g_j = sum_k b_jk^2, one thread per row of B, one fma per column, k ascending from an exact 0, into `work`.
 *   2. the search: a block owns 64 rows of A (four waves of one 16-row tile, staged once in LDS) and one SPLIT of B, a
 *      contiguous range of its 64-row panels, streamed through LDS; t_ij = a_i . b_j on v_mfma_f64_16x16x4_f64, one
 *      accumulator per (i, j), k ascending in steps of 4, four column tiles per wave and panel; s_ij = fma(-2, t_ij, g_j)
 *      depends on row i and row j alone, not on where they lie.  The running (score, index) of a row is carried in
 *      registers over the panels (a later column wins only with a strictly smaller score) and reduced over the 16 lanes
 *      of the row at the end: the smaller score, the lower index on equal scores.  One (score, index) per (row, split)
 *      goes to `work`.
 *   3. the merge, one thread per row of A: the splits in index order under the same rule give index[i]; then
 *      dist2[i] = sum_k (a_ik - b_jk)^2 for the winning j, the difference rounded once and fused into the sum, k
 *      ascending from 0: never negative, exactly 0 for equal rows, not derived from s.
 *   index      int64[nA]         argmin_j s_ij, the lowest j on equal scores.  In [0, nB) whatever the scores are: a score
 *                                that is not a number wins no comparison.
 *   dist2      double[nA]
 *   work       double[eaqhm_nn_work_len]   nB + 2 S nA words: g, then score and index (as a double, exact) per
 *                                (split, row)
 * The split count S = eaqhm_nn_splits(nA, nB) is a function of nA and nB alone, never of the device:
 *   S = min(ceil(nB / 4096), max(1, ceil(1024 / ceil(nA / 64))))
 *   (a split has at least 4096 rows of B, and splits are added until about 1024 blocks exist: four for each of 256 CUs).
 *   Split s owns the panels floor(s P / S) .. floor((s + 1) P / S) - 1 of the P = ceil(nB / 64) panels.
 * eaqhm_nn_splits and eaqhm_nn_work_len return -1 for sizes out of range.
 * The entry point does not read the device arrays: finite rows are the CALLER'S contract.
 * EAQHM_EINVAL, nothing launched, for null pointers, lda < D, ldb < D and sizes outside the ranges above.              */
int32_t eaqhm_nn_splits(int64_t nA, int64_t nB);
int64_t eaqhm_nn_work_len(int64_t nA, int64_t nB, int32_t D);
int eaqhm_nn_rows(eaqhm_ctx* ctx, const double* A, int64_t nA, int64_t lda, const double* B, int64_t nB, int64_t ldb,
                  int32_t D, double* work, int64_t* index, double* dist2);

#ifdef __cplusplus
}
#endif
#endif
