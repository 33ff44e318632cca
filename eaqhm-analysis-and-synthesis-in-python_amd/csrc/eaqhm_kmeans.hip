// eaqhm_kmeans.hip — the k-means codebook that starts the mixture of the spectral conversion.  gfx950
// (MI355X) only.
//
//   eaqhm_kmeans_assign_kernel  64 rows per block: z . c_m on the matrix pipe (v_mfma_f64_16x16x4_f64), the score
//                               fma(-2, z . c_m, g_m), its argmin over m (lowest index on ties), the rows that moved
//   eaqhm_kmeans_update_kernel  one block per row chunk, one thread per column: count, sum z and sum z o z per cluster in
//                               LDS, rows in row order; the chunk's sums go to `work`
//   eaqhm_kmeans_sum_kernel     adds the chunks in index order
//
// The MFMA's lane maps are those of eaqhm_gmm.hip: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; result register
// r of lane l is D[(l >> 4) + 4 r][l & 15].  Every operand comes from LDS, where rows and columns beyond the data are
// zeros: no kernel reads past the D columns of a row.  No atomics: every output word has one writer.
#include "eaqhm_common.h"
#include "eaqhm_gmm_chunks.h"

namespace eaqhm {

typedef long long i64;
typedef double kd4 __attribute__((ext_vector_type(4)));

constexpr int KM_DMAX = 128;        // columns at most
constexpr int KM_KMAX = 64;         // centres at most
constexpr int KM_ROWS = 64;         // rows of an assign block: four waves, one 16-row MFMA tile each
constexpr i64 KM_NMAX = ((i64)1 << 31) - 1;
constexpr int KM_UPDATE_THREADS = 128;
constexpr int KM_BATCH = 32;        // rows whose loads are in flight together in the update

// LDS row stride in doubles of the assign kernel: the 16 lanes of a quarter wave read 16 rows at the same k, the
// quarters k .. k + 3.  D padded to a multiple of 4, plus 2: half the stride is odd, so 16 rows x 2 columns of a half wave
// (the unit of a 64-bit LDS read) fall on 32 different even dword pairs: all 64 banks.
__host__ __device__ inline int km_pad4(int d) { return (d + 3) & ~3; }
__host__ __device__ inline int km_stride(int d) { return km_pad4(d) + 2; }
__host__ __device__ inline int km_pad16(int k) { return (k + 15) & ~15; }

// ------------------------------------------------------------------------------------------------
// The assignment.  LDS: Zs[64][LS] the block's rows, Cs[16][LS] one panel of 16 centres, gs[16 ceil(K / 16)] (+inf
// beyond K: such a score never wins), lab[64].  At D = 128, K = 64: 83 968 bytes, one block per CU; at D = 100, K = 32:
// 65 792, two; at D = 36, K = 8: 24 704, six.  Wave w owns rows 16 w .. 16 w + 15: t[n][m] = sum_k z_n[k] c_m[k] as
// A = z, B[k][m] = c_m[k].
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_kmeans_assign_kernel(const double* __restrict__ Z, i64 N, i64 ldz, int D, const double* __restrict__ C,
                               const double* __restrict__ g, int K, int* __restrict__ labels, int* __restrict__ changed) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int Dp = km_pad4(D), LS = km_stride(D), Kp = km_pad16(K);
  double* Zs = lds;
  double* Cs = Zs + KM_ROWS * LS;
  double* gs = Cs + 16 * LS;
  int* lab = (int*)(gs + Kp);
  const i64 n0 = (i64)blockIdx.x * KM_ROWS;
  const int rows = (int)(N - n0 < KM_ROWS ? N - n0 : KM_ROWS);
  for (int k = tid; k < KM_ROWS * Dp; k += 256) {
    const int r = k / Dp, j = k - r * Dp;
    Zs[r * LS + j] = r < rows && j < D ? Z[(size_t)(n0 + r) * ldz + j] : 0.0;
  }
  for (int m = tid; m < Kp; m += 256) gs[m] = m < K ? g[m] : INFINITY;
  double best[4] = {0.0, 0.0, 0.0, 0.0};
  int arg[4] = {0, 0, 0, 0};
  const double* zr = Zs + (16 * w + lr) * LS + lq;
  const double* cr = Cs + lr * LS + lq;
  for (int kp = 0; kp < Kp / 16; ++kp) {
    __syncthreads();   // Zs and gs are staged (kp = 0); the last panel is read
    for (int k = tid; k < 16 * Dp; k += 256) {
      const int r = k / Dp, j = k - r * Dp, m = 16 * kp + r;
      Cs[r * LS + j] = m < K && j < D ? C[(size_t)m * D + j] : 0.0;
    }
    __syncthreads();
    kd4 t = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < Dp; k0 += 4) t = __builtin_amdgcn_mfma_f64_16x16x4f64(zr[k0], cr[k0], t, 0, 0, 0);
    const int m = 16 * kp + lr;
    const double gm = gs[m];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double s = fma(-2.0, t[r], gm);
      if (kp == 0 || s < best[r]) {   // a later panel wins only with a smaller score
        best[r] = s;
        arg[r] = m;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {   // over the 16 lanes of a row: the smaller score, the lower index on equal scores
    for (int d = 1; d < 16; d <<= 1) {
      const double so = __shfl_xor(best[r], d);
      const int ao = __shfl_xor(arg[r], d);
      if (so < best[r] || (so == best[r] && ao < arg[r])) {
        best[r] = so;
        arg[r] = ao;
      }
    }
    // a NaN score (the caller's error) wins no comparison and could leave a padded lane's index: never a label >= K
    if (lr == 0) lab[16 * w + lq + 4 * r] = arg[r] < K ? arg[r] : 0;
  }
  __syncthreads();
  if (tid < KM_ROWS) {   // wave 0, one lane per row
    bool moved = false;
    if (tid < rows) {
      moved = labels[n0 + tid] != lab[tid];
      labels[n0 + tid] = lab[tid];
    }
    const unsigned long long mask = __ballot(moved);
    if (tid == 0) changed[blockIdx.x] = __popcll(mask);
  }
}

// ------------------------------------------------------------------------------------------------
// The update.  Block b owns chunk b; thread j < D owns column j.  LDS: S[K][D] and Q[K][D] doubles and cnt[K] of 64 bits,
// 131 584 bytes at K = 64, D = 128.  A row's label is the same for every thread, so the sums of the running cluster stay
// in registers and go back to LDS when the label changes: rows of one cluster that follow each other cost no LDS round
// trip, and the order of the additions is the row order either way.  The loads of KM_BATCH rows are issued together.
// work: [chunk][m][2 D + 1] = S1_m | Q_m | n_m (a count below 2^53 is exact as a double).
extern "C" __global__ void __launch_bounds__(KM_UPDATE_THREADS)
    eaqhm_kmeans_update_kernel(const double* __restrict__ Z, i64 N, i64 ldz, int D, const int* __restrict__ labels, int K,
                               i64 chunk_rows, double* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int j = threadIdx.x;
  double* S = lds;
  double* Q = S + K * D;
  double* cnt = Q + K * D;
  for (int k = j; k < 2 * K * D + K; k += KM_UPDATE_THREADS) lds[k] = 0.0;
  __syncthreads();
  const i64 c0 = (i64)blockIdx.x * chunk_rows, c1 = c0 + chunk_rows < N ? c0 + chunk_rows : N;
  if (j < D) {
    int cur = -1;
    double s = 0.0, q = 0.0, n = 0.0;
    for (i64 r0 = c0; r0 < c1; r0 += KM_BATCH) {
      double z[KM_BATCH];
      int l[KM_BATCH];
#pragma unroll
      for (int i = 0; i < KM_BATCH; ++i) {
        const bool in = r0 + i < c1;
        l[i] = in ? labels[r0 + i] : -1;
        z[i] = in ? Z[(size_t)(r0 + i) * ldz + j] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < KM_BATCH; ++i) {
        if (l[i] < 0 || l[i] >= K) continue;   // beyond the chunk, or the caller's error: skipped, never an index
        if (l[i] != cur) {
          if (cur >= 0) {
            S[cur * D + j] = s;
            Q[cur * D + j] = q;
            if (j == 0) cnt[cur] = n;
          }
          cur = l[i];
          s = S[cur * D + j];
          q = Q[cur * D + j];
          if (j == 0) n = cnt[cur];
        }
        s += z[i];
        q = fma(z[i], z[i], q);
        n += 1.0;
      }
    }
    if (cur >= 0) {
      S[cur * D + j] = s;
      Q[cur * D + j] = q;
      if (j == 0) cnt[cur] = n;
    }
  }
  __syncthreads();
  const int W = 2 * D + 1;
  double* out = work + (size_t)blockIdx.x * K * W;
  for (int k = j; k < K * W; k += KM_UPDATE_THREADS) {
    const int m = k / W, e = k - m * W;
    out[k] = e < D ? S[m * D + e] : e < 2 * D ? Q[m * D + e - D] : cnt[m];
  }
}

// One thread per output word: the chunks in index order.
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_kmeans_sum_kernel(const double* __restrict__ work, int n_chunks, int D, int K, i64* __restrict__ count,
                            double* __restrict__ S1, double* __restrict__ Q) {
  const int W = 2 * D + 1, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K * W) return;
  const int m = k / W, e = k - m * W;
  double v = 0.0;
  for (int c = 0; c < n_chunks; ++c) v += work[(size_t)c * K * W + k];
  if (e < D) {
    S1[(size_t)m * D + e] = v;
  } else if (e < 2 * D) {
    Q[(size_t)m * D + e - D] = v;
  } else {
    count[m] = (i64)v;
  }
}
}  // namespace eaqhm

using namespace eaqhm;

static bool km_sizes_ok(int64_t N, int32_t D, int32_t K) {
  return N >= 1 && N <= KM_NMAX && D >= 1 && D <= KM_DMAX && K >= 1 && K <= KM_KMAX;
}

extern "C" int64_t eaqhm_kmeans_work_len(int64_t N, int32_t D, int32_t K) {
  if (!km_sizes_ok(N, D, K)) return -1;
  const i64 R = gmm_chunk_rows(N);
  return (N + R - 1) / R * K * (2 * D + 1);
}

extern "C" int eaqhm_kmeans_assign(eaqhm_ctx* ctx, const double* Z, int64_t N, int64_t ldz, int32_t D, const double* C,
                                   const double* g, int32_t K, int32_t* labels, int32_t* changed) {
  if (!ctx) return EAQHM_EINVAL;
  if (!Z || !C || !g || !labels || !changed) return ctx->fail(EAQHM_EINVAL, "eaqhm_kmeans_assign: bad argument");
  if (!km_sizes_ok(N, D, K) || ldz < D)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_kmeans_assign: need 1 <= N < 2^31, 1 <= D <= 128, D <= ldz, 1 <= K <= 64");
  const size_t lds = ((size_t)(KM_ROWS + 16) * km_stride(D) + km_pad16(K)) * sizeof(double) + KM_ROWS * sizeof(int);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_kmeans_assign_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  hipLaunchKernelGGL(eaqhm_kmeans_assign_kernel, dim3((unsigned)((N + KM_ROWS - 1) / KM_ROWS)), dim3(256), lds,
                     ctx->stream, Z, (i64)N, (i64)ldz, (int)D, C, g, (int)K, labels, changed);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_kmeans_update(eaqhm_ctx* ctx, const double* Z, int64_t N, int64_t ldz, int32_t D,
                                   const int32_t* labels, int32_t K, double* work, int64_t* count, double* S1, double* Q) {
  if (!ctx) return EAQHM_EINVAL;
  if (!Z || !labels || !work || !count || !S1 || !Q) return ctx->fail(EAQHM_EINVAL, "eaqhm_kmeans_update: bad argument");
  if (!km_sizes_ok(N, D, K) || ldz < D)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_kmeans_update: need 1 <= N < 2^31, 1 <= D <= 128, D <= ldz, 1 <= K <= 64");
  const i64 R = gmm_chunk_rows(N);
  const int n_chunks = (int)((N + R - 1) / R);
  const size_t lds = ((size_t)2 * K * D + K) * sizeof(double);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_kmeans_update_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  hipLaunchKernelGGL(eaqhm_kmeans_update_kernel, dim3((unsigned)n_chunks), dim3(KM_UPDATE_THREADS), lds, ctx->stream, Z,
                     (i64)N, (i64)ldz, (int)D, labels, (int)K, R, work);
  hipLaunchKernelGGL(eaqhm_kmeans_sum_kernel, dim3((unsigned)((K * (2 * D + 1) + 255) / 256)), dim3(256), 0, ctx->stream,
                     work, n_chunks, (int)D, (int)K, (i64*)count, S1, Q);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
