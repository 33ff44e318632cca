/* eaqhm_kmeans.h — part of the C ABI of libeaqhm_hip.so (included by eaqhm_hip.h, which declares eaqhm_ctx and the
 * error codes): the k-means codebook that starts the mixture of the spectral conversion.                              */
#ifndef EAQHM_KMEANS_H
#define EAQHM_KMEANS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the two steps of a Lloyd round (additions under ABI 6) ----------------------------------------------
 * Rows Z double[N][ldz]: the first D <= ldz columns of a row are used, the others are never read (a mixture's centred
 * rows serve as they are, with D = split).  1 <= N < 2^31, 1 <= D <= 128, 1 <= K <= 64; none needs to be a multiple of
 * 4 or 16: the kernels pad in LDS.
 * eaqhm_kmeans_assign (kernel: 64 rows per block, four waves of one 16-row tile; the rows once and the centres in panels
 *   of 16 through LDS, zeros beyond D and K; t = z . c_m on v_mfma_f64_16x16x4_f64, one accumulator, k ascending, so
 *   every centre sees the same order of operations and equal centres give equal bits; the argmin is carried over the
 *   panels in registers and over the 16 lanes of a row at the end):
 *   C          double[K][D]      the centres
 *   g          double[K]         g_m = |c_m|^2, the CALLER'S numbers (the Python host forms them in float64)
 *   labels     int32[N]          in: the labels before, out: argmin_m s_nm, s_nm = fma(-2, t_nm, g_m); the lowest m on
 *                                equal scores.  In [0, K) whatever the scores are
 *                                (with a score that is not a number, which label is undefined).
 *   changed    int32[ceil(N / 64)]  per block of 64 rows, the number of rows whose label moved
 * eaqhm_kmeans_update (kernels: one block per chunk of R = max(512, 64 ceil(ceil(N / 128) / 64)) rows, the M-step's
 *   chunks, one thread per column: the sums of the chunk per cluster in LDS, the rows added in row order, the running
 *   cluster's sums in registers; then one thread per output word adds the chunks in index order.  No atomics, every
 *   word has one writer: the same bits on every run and every device):
 *   labels     int32[N]          a label outside [0, K) is the CALLER'S error: the row is skipped, nothing is indexed by it
 *   count      int64[K]          n_m, the rows of cluster m
 *   S1, Q      double[K][D]      S1_m = sum z, Q_m = sum z o z (each z^2 fused into its addition) over the rows of m
 *   work       double[eaqhm_kmeans_work_len]  ceil(N / R) K (2 D + 1) words; eaqhm_kmeans_work_len returns -1 for sizes
 *                                out of range
 * The entry points do not read the device arrays: finite rows and centres are the CALLER'S contract.
 * EAQHM_EINVAL, nothing launched, for null pointers, ldz < D and sizes outside the ranges above.                       */
int64_t eaqhm_kmeans_work_len(int64_t N, int32_t D, int32_t K);
int eaqhm_kmeans_assign(eaqhm_ctx* ctx, const double* Z, int64_t N, int64_t ldz, int32_t D, const double* C,
                        const double* g, int32_t K, int32_t* labels, int32_t* changed);
int eaqhm_kmeans_update(eaqhm_ctx* ctx, const double* Z, int64_t N, int64_t ldz, int32_t D, const int32_t* labels,
                        int32_t K, double* work, int64_t* count, double* S1, double* Q);

#ifdef __cplusplus
}
#endif
#endif
