// eaqhm_nn.hip — for every row of A the nearest row of B: the search of the non-parallel training.
// gfx950 (MI355X) only.
//
//   eaqhm_nn_norm_kernel    g_j = |b_j|^2, one thread per row of B
//   eaqhm_nn_search_kernel  a block owns 64 rows of A and one split of B: a . b on the matrix pipe
//                           (v_mfma_f64_16x16x4_f64), the score fma(-2, a . b, g), its argmin over the split (lowest index
//                           on ties); one (score, index) per (row, split) goes to `work`
//   eaqhm_nn_merge_kernel   one thread per row of A: the splits in index order, then the squared distance to the winner
//
// The MFMA's lane maps are those of eaqhm_kmeans.hip: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; result
// register r of lane l is D[(l >> 4) + 4 r][l & 15].  Every operand comes from LDS, where rows and columns beyond the data
// are zeros: no kernel reads past the D columns of a row.  No atomics: every output word has one writer.
#include "eaqhm_common.h"

namespace eaqhm {

typedef long long i64;
typedef double nd4 __attribute__((ext_vector_type(4)));

constexpr int NN_DMAX = 128;         // columns at most
constexpr int NN_ROWS = 64;          // rows of A of a search block: four waves, one 16-row MFMA tile each
constexpr int NN_PANEL = 64;         // rows of B of a panel: four column tiles, four accumulators per wave
constexpr int NN_BATCH = 8;          // loads of a thread in flight together while a tile is staged
constexpr i64 NN_NMAX = ((i64)1 << 31) - 1;
constexpr i64 NN_SPLIT_MIN = 4096;   // rows of B of a split at least
constexpr i64 NN_BLOCKS = 1024;      // splits are added until about this many blocks exist

// LDS row stride in doubles, the k-means kernel's: D padded to a multiple of 4, plus 2, so that half the stride is odd and
// the 16 rows x 2 columns of a half wave fall on all 64 banks.
__host__ __device__ inline int nn_pad4(int d) { return (d + 3) & ~3; }
__host__ __device__ inline int nn_stride(int d) { return nn_pad4(d) + 2; }

__host__ __device__ inline i64 nn_split_count(i64 nA, i64 nB) {
  const i64 by_rows = (nB + NN_SPLIT_MIN - 1) / NN_SPLIT_MIN, blocks = (nA + NN_ROWS - 1) / NN_ROWS;
  const i64 by_blocks = (NN_BLOCKS + blocks - 1) / blocks;   // >= 1
  return by_rows < by_blocks ? by_rows : by_blocks;
}

// Stages rows row0 .. row0 + 63 of X [n][ld] into dst[64][LS], zeros beyond row n and column D: consecutive threads take
// consecutive columns of a row, NN_BATCH loads of a thread are in flight together, and (row, column) advance by 256
// words a step without a division.
__device__ inline void nn_stage(double* __restrict__ dst, const double* __restrict__ X, i64 row0, i64 n, i64 ld, int D,
                                int Dp, int LS, int tid) {
  const int qd = 256 / Dp, rd = 256 - qd * Dp, words = NN_ROWS * Dp;
  int r = tid / Dp, j = tid - r * Dp;
  for (int k = tid; k < words; k += 256 * NN_BATCH) {
    double v[NN_BATCH];
    int at[NN_BATCH];
#pragma unroll
    for (int u = 0; u < NN_BATCH; ++u) {
      const bool in = k + 256 * u < words;
      at[u] = in ? r * LS + j : -1;
      v[u] = in && row0 + r < n && j < D ? X[(size_t)(row0 + r) * ld + j] : 0.0;
      j += rd;
      r += qd;
      if (j >= Dp) {
        j -= Dp;
        ++r;
      }
    }
#pragma unroll
    for (int u = 0; u < NN_BATCH; ++u)
      if (at[u] >= 0) dst[at[u]] = v[u];
  }
}

extern "C" __global__ void __launch_bounds__(256)
    eaqhm_nn_norm_kernel(const double* __restrict__ B, i64 nB, i64 ldb, int D, double* __restrict__ g) {
  const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
  if (j >= nB) return;
  const double* b = B + (size_t)j * ldb;
  double s = 0.0;
  for (int k = 0; k < D; ++k) s = fma(b[k], b[k], s);
  g[j] = s;
}

// ------------------------------------------------------------------------------------------------
// The search.  LDS: As[64][LS] the block's rows of A, Bs[64][LS] one panel of B, gs[64] (+inf beyond the split: such a
// score never wins a comparison).  At D = 128: 133 632 bytes, one block per CU; at D = 24: 27 136, six by LDS and four by
// registers.  Wave w owns rows
// 16 w .. 16 w + 15 of A and all 64 columns of the panel: t[c][i][j] = sum_k a_i[k] b_(16 c + j)[k], c = 0 .. 3.
// blockIdx.x: the 64 rows of A; blockIdx.y: the split, panels floor(y P / S) .. floor((y + 1) P / S) - 1.
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_nn_search_kernel(const double* __restrict__ A, i64 nA, i64 lda, const double* __restrict__ B, i64 nB, i64 ldb,
                           int D, const double* __restrict__ g, double* __restrict__ score, double* __restrict__ arg_out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int Dp = nn_pad4(D), LS = nn_stride(D);
  double* As = lds;
  double* Bs = As + NN_ROWS * LS;
  double* gs = Bs + NN_PANEL * LS;
  const i64 n0 = (i64)blockIdx.x * NN_ROWS;
  const int rows = (int)(nA - n0 < NN_ROWS ? nA - n0 : NN_ROWS);
  const i64 P = (nB + NN_PANEL - 1) / NN_PANEL, S = gridDim.y, sp = blockIdx.y;
  const i64 p0 = sp * P / S, p1 = (sp + 1) * P / S;   // S <= P: no split is empty
  nn_stage(As, A, n0, nA, lda, D, Dp, LS, tid);
  // +inf and the split's first row before any score: a score wins only by being smaller, so equal scores keep the lowest
  // index, and one that is not a number (the caller's error) wins nothing: the index stays inside the split
  double best[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
  i64 arg[4] = {p0 * NN_PANEL, p0 * NN_PANEL, p0 * NN_PANEL, p0 * NN_PANEL};
  const double* ar = As + (16 * w + lr) * LS + lq;
  const double* br = Bs + lr * LS + lq;
  for (i64 p = p0; p < p1; ++p) {
    const i64 j0 = p * NN_PANEL;
    __syncthreads();   // the last panel is read
    nn_stage(Bs, B, j0, nB, ldb, D, Dp, LS, tid);
    if (tid < NN_PANEL) gs[tid] = j0 + tid < nB ? g[j0 + tid] : INFINITY;
    __syncthreads();   // As (first panel), Bs and gs are staged
    nd4 t0 = {0.0, 0.0, 0.0, 0.0}, t1 = t0, t2 = t0, t3 = t0;
    for (int k0 = 0; k0 < Dp; k0 += 4) {
      const double a = ar[k0];
      t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, br[k0], t0, 0, 0, 0);
      t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, br[16 * LS + k0], t1, 0, 0, 0);
      t2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, br[32 * LS + k0], t2, 0, 0, 0);
      t3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, br[48 * LS + k0], t3, 0, 0, 0);
    }
    const nd4 t[4] = {t0, t1, t2, t3};
#pragma unroll
    for (int c = 0; c < 4; ++c) {   // the column tiles in index order
      const double gj = gs[16 * c + lr];
      const i64 j = j0 + 16 * c + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double s = fma(-2.0, t[c][r], gj);
        const bool take = s < best[r];   // a later column wins only with a smaller score
        best[r] = take ? s : best[r];
        arg[r] = take ? j : arg[r];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {   // over the 16 lanes of a row: the smaller score, the lower index on equal scores
    for (int d = 1; d < 16; d <<= 1) {
      const double so = __shfl_xor(best[r], d);
      const i64 ao = __shfl_xor(arg[r], d);
      const bool take = so < best[r] || (so == best[r] && ao < arg[r]);
      best[r] = take ? so : best[r];
      arg[r] = take ? ao : arg[r];
    }
    const int i = 16 * w + lq + 4 * r;
    if (lr == 0 && i < rows) {
      score[(size_t)sp * nA + n0 + i] = best[r];
      arg_out[(size_t)sp * nA + n0 + i] = (double)arg[r];   // below 2^31: exact
    }
  }
}

// One thread per row of A: the splits in index order, then the squared distance to the winner from the rows themselves.
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_nn_merge_kernel(const double* __restrict__ A, i64 nA, i64 lda, const double* __restrict__ B, i64 ldb, int D,
                          int S, const double* __restrict__ score, const double* __restrict__ arg_in,
                          i64* __restrict__ index, double* __restrict__ dist2) {
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  if (i >= nA) return;
  double best = score[i];
  i64 arg = (i64)arg_in[i];
  for (int s = 1; s < S; ++s) {
    const double so = score[(size_t)s * nA + i];
    const i64 ao = (i64)arg_in[(size_t)s * nA + i];
    if (so < best || (so == best && ao < arg)) {
      best = so;
      arg = ao;
    }
  }
  index[i] = arg;
  const double* a = A + (size_t)i * lda;
  const double* b = B + (size_t)arg * ldb;
  double d2 = 0.0;
  for (int k = 0; k < D; ++k) {
    const double d = a[k] - b[k];
    d2 = fma(d, d, d2);
  }
  dist2[i] = d2;
}
}  // namespace eaqhm

using namespace eaqhm;

static bool nn_sizes_ok(int64_t nA, int64_t nB) { return nA >= 1 && nA <= NN_NMAX && nB >= 1 && nB <= NN_NMAX; }

extern "C" int32_t eaqhm_nn_splits(int64_t nA, int64_t nB) {
  return nn_sizes_ok(nA, nB) ? (int32_t)nn_split_count(nA, nB) : -1;
}

extern "C" int64_t eaqhm_nn_work_len(int64_t nA, int64_t nB, int32_t D) {
  if (!nn_sizes_ok(nA, nB) || D < 1 || D > NN_DMAX) return -1;
  return nB + 2 * nn_split_count(nA, nB) * nA;
}

extern "C" int eaqhm_nn_rows(eaqhm_ctx* ctx, const double* A, int64_t nA, int64_t lda, const double* B, int64_t nB,
                             int64_t ldb, int32_t D, double* work, int64_t* index, double* dist2) {
  if (!ctx) return EAQHM_EINVAL;
  if (!A || !B || !work || !index || !dist2) return ctx->fail(EAQHM_EINVAL, "eaqhm_nn_rows: bad argument");
  if (!nn_sizes_ok(nA, nB) || D < 1 || D > NN_DMAX || lda < D || ldb < D)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_nn_rows: need 1 <= nA, nB < 2^31, 1 <= D <= 128, D <= lda, D <= ldb");
  const int S = (int)nn_split_count(nA, nB);
  double* g = work;
  double* score = work + nB;
  double* arg = score + (size_t)S * nA;
  const size_t lds = ((size_t)(NN_ROWS + NN_PANEL) * nn_stride(D) + NN_PANEL) * sizeof(double);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_nn_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  hipLaunchKernelGGL(eaqhm_nn_norm_kernel, dim3((unsigned)((nB + 255) / 256)), dim3(256), 0, ctx->stream, B, (i64)nB,
                     (i64)ldb, (int)D, g);
  hipLaunchKernelGGL(eaqhm_nn_search_kernel, dim3((unsigned)((nA + NN_ROWS - 1) / NN_ROWS), (unsigned)S), dim3(256), lds,
                     ctx->stream, A, (i64)nA, (i64)lda, B, (i64)nB, (i64)ldb, (int)D, (const double*)g, score, arg);
  hipLaunchKernelGGL(eaqhm_nn_merge_kernel, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, ctx->stream, A, (i64)nA,
                     (i64)lda, B, (i64)ldb, (int)D, S, (const double*)score, (const double*)arg, (i64*)index, dist2);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
