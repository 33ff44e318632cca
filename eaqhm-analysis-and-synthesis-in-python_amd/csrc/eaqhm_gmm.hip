// eaqhm_gmm.hip — the joint-density Gaussian mixture of the spectral conversion.  gfx950 (MI355X) only,
// FP64 on the matrix pipe (v_mfma_f64_16x16x4_f64).
//
//   eaqhm_gmm_estep_kernel    64 rows per block: q = ||W_m (c - mu_m)||^2 over the lower triangle of W_m, log-sum-exp
//                             over the components and the responsibilities, one launch
//   eaqhm_gmm_mstep_kernel    one (row chunk, component) per block: the weighted Gramian of [c | 1] over the lower-
//                             triangle 16 x 16 tiles, S1 and S0 in its last row; the chunk's tiles go to `work`
//   eaqhm_gmm_msum_kernel     adds the chunks in index order, mirrors S2, splits off S1 and S0
//   eaqhm_gmm_regress_kernel  64 rows per block: X A_m^T + b_m on the matrix pipe, weighted by gamma and summed over m
//
// The MFMA's lane maps are in eaqhm_gmm_mfma.h, with the tile, the stride rules and the 16-lane sum that the conditional
// E-step (eaqhm_mlpg_em.hip) shares.  Every operand comes from LDS, where rows and columns beyond the data are
// zeros: no kernel reads past a row of its arguments.  No atomics: every output word has one writer.
#include "eaqhm_common.h"
#include "eaqhm_gmm_mfma.h"

namespace eaqhm {

typedef long long i64;

constexpr int GMM_DMAX = 128;    // columns of Z at most
constexpr int GMM_XMAX = 64;     // dx, dy at most
constexpr int GMM_MMAX = 64;     // components at most
constexpr i64 GMM_NMAX = (i64)1 << 36;
constexpr int GMM_TILES_PER_WAVE = 12;   // ceil(45 / 4): D + 1 = 129 columns are 9 tile rows, 45 lower tiles

// (the M-step's chunking, gmm_chunk_rows, is in eaqhm_gmm_chunks.h)
__host__ __device__ inline int gmm_tiles(int D) {
  const int nt = (D + 1 + 15) / 16;
  return nt * (nt + 1) / 2;
}

// ------------------------------------------------------------------------------------------------
// The E-step.  LDS (doubles): Zs[64][LS] the block's rows, Ws[16][LS] one 16-row panel of W_m (entries above the
// diagonal and beyond D as zeros, whatever the argument holds there), mus[LS], lp[64][M | 1], srow[64].
// At D = 128, M = 64: 118 032 bytes, one block per CU; at D = 36, M = 8: 47 888 bytes, three.
// Wave w owns rows 16 w .. 16 w + 15.  Panel kp of W_m (rows 16 kp .. 16 kp + 15) is contracted over its columns
// 0 .. 16 kp + 15 only: y[n][k] = sum_j (c_n[j] - mu[j]) W[k][j] as A = c - mu, B[j][k] = W[k][j], two accumulators.
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_gmm_estep_kernel(const double* __restrict__ Z, i64 N, int D, int M, const double* __restrict__ mu,
                           const double* __restrict__ W, const double* __restrict__ kk, double* __restrict__ gamma,
                           double* __restrict__ ll) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int Dp = gmm_pad16(D), LS = gmm_stride_rowk(D), LM = M | 1;
  double* Zs = lds;
  double* Ws = Zs + GMM_ROWS * LS;
  double* mus = Ws + 16 * LS;
  double* lp = mus + LS;
  double* srow = lp + GMM_ROWS * LM;
  const i64 n0 = (i64)blockIdx.x * GMM_ROWS;
  const int rows = (int)(N - n0 < GMM_ROWS ? N - n0 : GMM_ROWS);
  for (int k = tid; k < GMM_ROWS * Dp; k += 256) {
    const int r = k / Dp, j = k - r * Dp;
    Zs[r * LS + j] = r < rows && j < D ? Z[(size_t)(n0 + r) * D + j] : 0.0;
  }
  for (int m = 0; m < M; ++m) {
    __syncthreads();   // Zs is staged (m = 0); the last component's mus and Ws are read
    for (int j = tid; j < Dp; j += 256) mus[j] = j < D ? mu[(size_t)m * D + j] : 0.0;
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    for (int kp = 0; kp < Dp / 16; ++kp) {
      const int jmax = 16 * kp + 16;
      if (kp) __syncthreads();   // the last panel is read
      for (int k = tid; k < 16 * jmax; k += 256) {
        const int r = k / jmax, j = k - r * jmax, row = 16 * kp + r;
        Ws[r * LS + j] = row < D && j <= row ? W[((size_t)m * D + row) * D + j] : 0.0;
      }
      __syncthreads();
      gd4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
      const double* zr = Zs + (16 * w + lr) * LS + lq;
      const double* wr = Ws + lr * LS + lq;
      for (int j0 = 0; j0 < jmax; j0 += 8) {
        acc0 = gmm_mfma(zr[j0] - mus[j0 + lq], wr[j0], acc0);
        acc1 = gmm_mfma(zr[j0 + 4] - mus[j0 + 4 + lq], wr[j0 + 4], acc1);
      }
      for (int r = 0; r < 4; ++r) {
        const double y = acc0[r] + acc1[r];
        q[r] = fma(y, y, q[r]);
      }
    }
    const double km = kk[m];
    for (int r = 0; r < 4; ++r) {
      const double qs = gmm_sum16(q[r]);
      if (lr == 0) lp[(16 * w + lq + 4 * r) * LM + m] = km - 0.5 * qs;
    }
  }
  __syncthreads();
  if (tid < rows) {   // one lane per row: the largest lp, e = exp(lp - max) in place, their sum
    double* p = lp + tid * LM;
    double mx = p[0];
    for (int m = 1; m < M; ++m) mx = fmax(mx, p[m]);
    double s = 0.0;
    // every q overflowed (a row some 1e154 standard deviations away): lp = max = -inf, and -inf - -inf is NaN.
    // Such a row has ll = -inf and no preference: gamma = 1 / M
    const bool lost = mx == -INFINITY;
    for (int m = 0; m < M; ++m) {
      const double e = lost ? 1.0 : exp(p[m] - mx);
      p[m] = e;
      s += e;
    }
    srow[tid] = s;
    ll[n0 + tid] = lost ? -INFINITY : mx + log(s);
  }
  __syncthreads();
  for (int k = tid; k < rows * M; k += 256) {   // gamma = e / s: a row sums to 1 within the roundings of the quotients
    const int r = k / M, m = k - r * M;
    gamma[(size_t)n0 * M + k] = lp[r * LM + m] / srow[r];
  }
}

// ------------------------------------------------------------------------------------------------
// The M-step.  Block b = chunk * M + m adds gamma_nm c'_n c'_n^T over its chunk's rows, c' = [c | 1 | 0 ..] of
// D + 1 columns padded to 16 nt: entry (D, j) is S1[j], (D, D) is S0.  Lower-triangle tile t = ti (ti + 1) / 2 + tj,
// tj <= ti, belongs to wave t & 3, slot t >> 2; its operands are A[i][n] = gamma_n c'_n[16 ti + i] and B[n][j] =
// c'_n[16 tj + j], four rows n per MFMA.  LDS: Cs[64][LS] and gs[64]: 74 240 bytes at D = 128, 25 088 at D = 36; two
// blocks per CU either way (176 VGPRs: two waves per SIMD).  Rows beyond the chunk are zeros.  The order of the
// additions is the row order: fixed.
__device__ inline void gmm_tile_coords(int t, int& ti, int& tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}

extern "C" __global__ void __launch_bounds__(256)
    eaqhm_gmm_mstep_kernel(const double* __restrict__ Z, const double* __restrict__ gamma, i64 N, int D, int M,
                           i64 chunk_rows, double* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // the tile tests below are scalar
  const int Dp = gmm_pad16(D + 1), LS = gmm_stride_krow(Dp), T = gmm_tiles(D);
  double* Cs = lds;
  double* gs = Cs + GMM_ROWS * LS;
  const i64 chunk = blockIdx.x / M;
  const int m = (int)(blockIdx.x - chunk * M);
  const i64 c0 = chunk * chunk_rows, c1 = c0 + chunk_rows < N ? c0 + chunk_rows : N;
  int oa[GMM_TILES_PER_WAVE], ob[GMM_TILES_PER_WAVE];
  gd4 acc[GMM_TILES_PER_WAVE];
#pragma unroll
  for (int s = 0; s < GMM_TILES_PER_WAVE; ++s) {
    int ti = 0, tj = 0;
    if (w + 4 * s < T) gmm_tile_coords(w + 4 * s, ti, tj);
    oa[s] = 16 * ti + lr;
    ob[s] = 16 * tj + lr;
    acc[s] = gd4{0.0, 0.0, 0.0, 0.0};
  }
  for (i64 r0 = c0; r0 < c1; r0 += GMM_ROWS) {
    __syncthreads();   // the last rows are read
    for (int k = tid; k < GMM_ROWS * Dp; k += 256) {
      const int r = k / Dp, j = k - r * Dp;
      double v = 0.0;
      if (r0 + r < c1) v = j < D ? Z[(size_t)(r0 + r) * D + j] : j == D ? 1.0 : 0.0;
      Cs[r * LS + j] = v;
    }
    if (tid < GMM_ROWS) gs[tid] = r0 + tid < c1 ? gamma[(size_t)(r0 + tid) * M + m] : 0.0;
    __syncthreads();
    for (int ks = 0; ks < GMM_ROWS / 4; ++ks) {
      const double g = gs[4 * ks + lq];
      const double* row = Cs + (4 * ks + lq) * LS;
#pragma unroll
      for (int s = 0; s < GMM_TILES_PER_WAVE; ++s)
        if (w + 4 * s < T) acc[s] = gmm_mfma(g * row[oa[s]], row[ob[s]], acc[s]);
    }
  }
  double* out = work + (size_t)blockIdx.x * T * 256;
#pragma unroll
  for (int s = 0; s < GMM_TILES_PER_WAVE; ++s)
    if (w + 4 * s < T)
      for (int r = 0; r < 4; ++r) out[(size_t)(w + 4 * s) * 256 + (lq + 4 * r) * 16 + lr] = acc[s][r];
}

// One thread per entry of a component's lower tiles: the chunks in index order, then S2[i][j] and its mirror, S1, S0.
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_gmm_msum_kernel(const double* __restrict__ work, int n_chunks, int D, int M, double* __restrict__ S0,
                          double* __restrict__ S1, double* __restrict__ S2) {
  const int T = gmm_tiles(D);
  const int m = blockIdx.x / T, t = blockIdx.x - m * T, e = threadIdx.x;
  int ti, tj;
  gmm_tile_coords(t, ti, tj);
  const int i = 16 * ti + (e >> 4), j = 16 * tj + (e & 15);
  if (i > D || j > i) return;   // padding; the upper half of a diagonal tile (its mirror is written instead)
  double v = 0.0;
  for (int c = 0; c < n_chunks; ++c) v += work[(((size_t)c * M + m) * T + t) * 256 + e];
  if (i < D) {
    S2[((size_t)m * D + i) * D + j] = v;
    S2[((size_t)m * D + j) * D + i] = v;
  } else if (j < D) {
    S1[(size_t)m * D + j] = v;
  } else {
    S0[m] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// The regression.  LDS: Xs[64][LS] the block's rows (dx padded to a multiple of 4 with zeros), As[16 njp][LS] the rows
// of A_m (rows beyond dy zeros), bs[16 njp], gs[64][M | 1]: 101 376 bytes at dx = dy = M = 64 (one block per CU),
// 30 976 at dx = dy = 18, M = 8 (five).  Wave w owns rows 16 w .. 16 w + 15 and all of their dy columns, in panels of 16:
// t[n][j] = sum_k x_n[k] A_m[j][k] on the matrix pipe, then y[n][j] += gamma_nm (t[n][j] + b_m[j]), m ascending.
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_gmm_regress_kernel(const double* __restrict__ X, const double* __restrict__ gamma, const double* __restrict__ A,
                             const double* __restrict__ b, i64 N, int dx, int dy, int M, double* __restrict__ Y) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int dxp = (dx + 3) & ~3, dyp = gmm_pad16(dy), njp = dyp / 16, LS = gmm_stride_rowk(dx), LM = M | 1;
  double* Xs = lds;
  double* As = Xs + GMM_ROWS * LS;
  double* bs = As + dyp * LS;
  double* gs = bs + dyp;
  const i64 n0 = (i64)blockIdx.x * GMM_ROWS;
  const int rows = (int)(N - n0 < GMM_ROWS ? N - n0 : GMM_ROWS);
  for (int k = tid; k < GMM_ROWS * dxp; k += 256) {
    const int r = k / dxp, j = k - r * dxp;
    Xs[r * LS + j] = r < rows && j < dx ? X[(size_t)(n0 + r) * dx + j] : 0.0;
  }
  for (int k = tid; k < GMM_ROWS * M; k += 256) {
    const int r = k / M, m = k - r * M;
    gs[r * LM + m] = r < rows ? gamma[(size_t)n0 * M + k] : 0.0;
  }
  gd4 y[4];
#pragma unroll
  for (int jp = 0; jp < 4; ++jp) y[jp] = gd4{0.0, 0.0, 0.0, 0.0};
  const double* xr = Xs + (16 * w + lr) * LS + lq;
  for (int m = 0; m < M; ++m) {
    __syncthreads();   // Xs and gs are staged (m = 0); the last component's As and bs are read
    for (int k = tid; k < dyp * dxp; k += 256) {
      const int r = k / dxp, j = k - r * dxp;
      As[r * LS + j] = r < dy && j < dx ? A[((size_t)m * dy + r) * dx + j] : 0.0;
    }
    for (int j = tid; j < dyp; j += 256) bs[j] = j < dy ? b[(size_t)m * dy + j] : 0.0;
    __syncthreads();
    double g[4];
    for (int r = 0; r < 4; ++r) g[r] = gs[(16 * w + lq + 4 * r) * LM + m];
#pragma unroll
    for (int jp = 0; jp < 4; ++jp)
      if (jp < njp) {
        gd4 t = {0.0, 0.0, 0.0, 0.0};
        const double* ar = As + (16 * jp + lr) * LS + lq;
        for (int k0 = 0; k0 < dxp; k0 += 4) t = gmm_mfma(xr[k0], ar[k0], t);
        const double bj = bs[16 * jp + lr];
        for (int r = 0; r < 4; ++r) y[jp][r] = fma(g[r], t[r] + bj, y[jp][r]);
      }
  }
#pragma unroll
  for (int jp = 0; jp < 4; ++jp)
    if (jp < njp)
      for (int r = 0; r < 4; ++r) {
        const int n = 16 * w + lq + 4 * r, j = 16 * jp + lr;
        if (n < rows && j < dy) Y[(size_t)(n0 + n) * dy + j] = y[jp][r];
      }
}
}  // namespace eaqhm

using namespace eaqhm;

static bool gmm_sizes_ok(int64_t N, int32_t D, int32_t M, int dmax) {
  return N >= 1 && N <= GMM_NMAX && D >= 1 && D <= dmax && M >= 1 && M <= GMM_MMAX;
}

extern "C" int64_t eaqhm_gmm_work_len(int64_t N, int32_t D, int32_t M) {
  if (!gmm_sizes_ok(N, D, M, GMM_DMAX)) return -1;
  const i64 R = gmm_chunk_rows(N);
  return (N + R - 1) / R * M * gmm_tiles(D) * 256;
}

extern "C" int eaqhm_gmm_estep(eaqhm_ctx* ctx, const double* Z, int64_t N, int32_t D, int32_t M, const double* mu,
                               const double* W, const double* k, double* gamma_out, double* ll_out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!Z || !mu || !W || !k || !gamma_out || !ll_out) return ctx->fail(EAQHM_EINVAL, "eaqhm_gmm_estep: bad argument");
  if (!gmm_sizes_ok(N, D, M, GMM_DMAX))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_gmm_estep: need 1 <= N <= 2^36, 1 <= D <= 128, 1 <= M <= 64");
  const int LS = gmm_stride_rowk(D);
  const size_t lds = ((size_t)(GMM_ROWS + 16 + 1) * LS + (size_t)GMM_ROWS * (M | 1) + GMM_ROWS) * sizeof(double);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_gmm_estep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  hipLaunchKernelGGL(eaqhm_gmm_estep_kernel, dim3((unsigned)((N + GMM_ROWS - 1) / GMM_ROWS)), dim3(256), lds,
                     ctx->stream, Z, (i64)N, (int)D, (int)M, mu, W, k, gamma_out, ll_out);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_gmm_mstep(eaqhm_ctx* ctx, const double* Z, const double* gamma, int64_t N, int32_t D, int32_t M,
                               double* work, double* S0, double* S1, double* S2) {
  if (!ctx) return EAQHM_EINVAL;
  if (!Z || !gamma || !work || !S0 || !S1 || !S2) return ctx->fail(EAQHM_EINVAL, "eaqhm_gmm_mstep: bad argument");
  if (!gmm_sizes_ok(N, D, M, GMM_DMAX))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_gmm_mstep: need 1 <= N <= 2^36, 1 <= D <= 128, 1 <= M <= 64");
  const i64 R = gmm_chunk_rows(N);
  const int n_chunks = (int)((N + R - 1) / R);
  const size_t lds = ((size_t)GMM_ROWS * gmm_stride_krow(gmm_pad16(D + 1)) + GMM_ROWS) * sizeof(double);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_gmm_mstep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  hipLaunchKernelGGL(eaqhm_gmm_mstep_kernel, dim3((unsigned)(n_chunks * M)), dim3(256), lds, ctx->stream, Z, gamma,
                     (i64)N, (int)D, (int)M, R, work);
  hipLaunchKernelGGL(eaqhm_gmm_msum_kernel, dim3((unsigned)(M * gmm_tiles(D))), dim3(256), 0, ctx->stream, work,
                     n_chunks, (int)D, (int)M, S0, S1, S2);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_gmm_regress(eaqhm_ctx* ctx, const double* X, const double* gamma, const double* A, const double* b,
                                 int64_t N, int32_t dx, int32_t dy, int32_t M, double* Y_out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!X || !gamma || !A || !b || !Y_out) return ctx->fail(EAQHM_EINVAL, "eaqhm_gmm_regress: bad argument");
  if (!gmm_sizes_ok(N, dx, M, GMM_XMAX) || dy < 1 || dy > GMM_XMAX)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_gmm_regress: need 1 <= N <= 2^36, 1 <= dx, dy <= 64, 1 <= M <= 64");
  const int LS = gmm_stride_rowk(dx), dyp = gmm_pad16(dy);
  const size_t lds = ((size_t)(GMM_ROWS + dyp) * LS + dyp + (size_t)GMM_ROWS * (M | 1)) * sizeof(double);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_gmm_regress_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  hipLaunchKernelGGL(eaqhm_gmm_regress_kernel, dim3((unsigned)((N + GMM_ROWS - 1) / GMM_ROWS)), dim3(256), lds,
                     ctx->stream, X, gamma, A, b, (i64)N, (int)dx, (int)dy, (int)M, Y_out);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
