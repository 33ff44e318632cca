// eaqhm_mlpg.hip — delta features of cepstral rows and the maximum-likelihood trajectory of the spectral conversion
// (DESIGN.md §12.1).  gfx950 (MI355X) only, FP64 on the vector pipe.
//
//   eaqhm_ceps_delta_kernel   one thread per entry (t, j): the regression window over the row's own run, clipped at its edges
//   eaqhm_mlpg_band_kernel    one thread per (row, column) of a run: row i of the band of R = diag(P^s) + W^T diag(P^D) W
//                             (entries R[i][i - k], k = 0 .. 2 span) and q_i = r^s_i + (W^T r^D)_i, into `work`
//   eaqhm_mlpg_solve_kernel   one lane per system (run, column): the root-free banded Cholesky R = L D L^T row by row, the
//                             forward substitution in the same sweep, then the backward sweep; L and D replace R in `work`
//
// Rows are [t][d]: the lanes of a wave are consecutive columns d of one run and read consecutive doubles.  A system is
// sequential in t; the window of the last b rows of L that row i needs lives in LDS, one private strip per lane
// ([entry][lane]: lane-consecutive doubles, no bank conflict, no barrier), so a run of any length needs the same LDS.
// Both sweeps take `work` in chunks of 8 rows through the same strip: the chunk's loads are issued together.
// Every index into a per-lane array is an LDS address: no scratch.  No atomics, every word has one writer, the order of
// every sum is fixed: the same input gives the same bits.
#include "eaqhm_mlpg_band.h"

namespace eaqhm {

constexpr int MLPG_CHUNK = 8;            // rows of `work` a lane stages into its LDS strip at a time

__host__ __device__ inline int mlpg_window(int b) { return (b > 0 ? b : 1) * (b + 1) + 2 * (b + 1) + (b > 0 ? b : 1); }
// lanes of a solve block and doubles of its LDS: 64 lanes while span <= 2 (41 984 bytes at span 2), 32 while span <= 4
// (45 568 at 4), 16 beyond (59 648 at 8): under the 64 KB a block gets without asking
__host__ __device__ inline int mlpg_lanes(int span) { return span <= 2 ? 64 : span <= 4 ? 32 : 16; }
__host__ __device__ inline size_t mlpg_lds_doubles(int span) {
  return (size_t)(mlpg_window(2 * span) + MLPG_CHUNK * mlpg_slots(span)) * mlpg_lanes(span);
}
// ------------------------------------------------------------------------------------------------
// Delta rows.  A row's run is found from column 0 of at most `span` neighbours on each side; beyond the run's edge the
// edge row is repeated (the HTK convention).  tau ascending.  An empty row, (-inf, ..), gets zeros.
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_ceps_delta_kernel(const double* __restrict__ C, i64 n, int cols, int span, double* __restrict__ out) {
  const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * cols) return;
  const i64 t = idx / cols;
  const int j = (int)(idx - t * cols);
  if (C[(size_t)t * cols] == -INFINITY) {
    out[idx] = 0.0;
    return;
  }
  i64 lo = t, hi = t;
  for (int tau = 1; tau <= span; ++tau) {
    if (t - tau < 0 || C[(size_t)(t - tau) * cols] == -INFINITY) break;
    lo = t - tau;
  }
  for (int tau = 1; tau <= span; ++tau) {
    if (t + tau >= n || C[(size_t)(t + tau) * cols] == -INFINITY) break;
    hi = t + tau;
  }
  const double den = mlpg_denominator(span);
  double acc = 0.0;
  for (int tau = 1; tau <= span; ++tau) {
    const i64 tp = t + tau < hi ? t + tau : hi, tm = t - tau > lo ? t - tau : lo;
    acc = fma((double)tau / den, C[(size_t)tp * cols + j] - C[(size_t)tm * cols + j], acc);
  }
  out[idx] = acc;
}

// ------------------------------------------------------------------------------------------------
// `count` doubles of a lane's column of `work` (stride dy) into its LDS strip (stride lanes): the loads of a batch are
// independent, so a chunk waits for the memory about once, not once per entry
__device__ inline void mlpg_stage(double* st, int lanes, const double* g, int dy, int count) {
#pragma unroll 8
  for (int e = 0; e < count; ++e) st[e * lanes] = g[(size_t)e * dy];
}

// x mod bw for x in [-bw, 2 bw)
__device__ inline int mlpg_ring(int x, int bw) { return x < 0 ? x + bw : x >= bw ? x - bw : x; }

// work[(t S + k) dy + d], S = 2 span + 2: k = 0 .. 2 span holds R[i][i - k] (i the row's index in its run, entries with
// i - k < 0 are not written or read), k = 2 span + 1 holds q_i.  u ascending in every sum.
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_mlpg_band_kernel(const double* __restrict__ P, const double* __restrict__ r, i64 n, int dy, int span,
                           const i64* __restrict__ run_start, const i64* __restrict__ run_len, i64 n_runs,
                           double* __restrict__ work) {
  const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * dy) return;
  const i64 t = idx / dy;
  const int d = (int)(idx - t * dy);
  const i64 run = mlpg_find_run(run_start, run_len, n_runs, n, t);
  if (run < 0) return;
  const i64 s = run_start[run], T = run_len[run], i = t - s;
  const int S = mlpg_slots(span), b = (int)(2 * span < T - 1 ? 2 * span : T - 1);
  const double den = mlpg_denominator(span);
  const size_t row = (size_t)2 * dy;
  const i64 u0 = i - span > 0 ? i - span : 0;
  double* w = work + (size_t)t * S * dy + d;
  const int kmax = (int)(i < b ? i : b);
  for (int k = 0; k <= kmax; ++k) {
    const i64 j = i - k, u1 = j + span < T - 1 ? j + span : T - 1;
    double acc = k == 0 ? P[(size_t)t * row + d] : 0.0;
    for (i64 u = u0; u <= u1; ++u)
      acc = fma(mlpg_coef(u, i, T, span, den) * mlpg_coef(u, j, T, span, den), P[(size_t)(s + u) * row + dy + d], acc);
    w[(size_t)k * dy] = acc;
  }
  const i64 u1 = i + span < T - 1 ? i + span : T - 1;
  double acc = r[(size_t)t * row + d];
  for (i64 u = u0; u <= u1; ++u) acc = fma(mlpg_coef(u, i, T, span, den), r[(size_t)(s + u) * row + dy + d], acc);
  w[(size_t)(S - 1) * dy] = acc;
}

// ------------------------------------------------------------------------------------------------
// Block (run, group of `lanes` columns), one lane per system.  b = min(2 span, T - 1).  Per-lane LDS strip, entry e of
// lane l at lds[e * lanes + l]:
//   Lw[bw][b + 1]  row j of the factor at slot j % bw: [0] = D_j, [k] = L[j][j - k]       (bw = max(b, 1))
//   ct[b + 1], cl[b + 1]  row i under construction: t_ik = L[i][i - k] D_(i - k) and L[i][i - k]
//   zw[bw]         the last b values of the forward sweep, then the pending sums of the backward sweep
//   st[8][2 span + 2]  the chunk of 8 rows of `work` being processed
// Row i: for j = i - kmax .. i - 1: t_ij = R_ij - sum_(m < j) t_im L_jm, L_ij = t_ij / D_j; D_i = R_ii - sum_m t_im L_im;
// z_i = q_i - sum_m L_im z_m; m ascending everywhere.  Back: y_i = z_i / D_i + (-sum_(k >= 1) L[i + k][i] y_(i + k)), k
// descending.  With P^D = 0 this is y_i = r^s_i / P^s_i, one rounding.
extern "C" __global__ void
    eaqhm_mlpg_solve_kernel(i64 n, int dy, int span, const i64* __restrict__ run_start, const i64* __restrict__ run_len,
                            double* __restrict__ work, double* __restrict__ Y) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lanes = blockDim.x, lane = threadIdx.x, d = blockIdx.y * lanes + lane;
  const i64 s = run_start[blockIdx.x], T = run_len[blockIdx.x];
  if (d >= dy || s < 0 || T < 1 || T > n || s > n - T) return;
  const int S = mlpg_slots(span), b = (int)(2 * span < T - 1 ? 2 * span : T - 1), bw = b > 0 ? b : 1;
  double* Lw = lds + lane;
  double* ct = Lw + (size_t)bw * (b + 1) * lanes;
  double* cl = ct + (size_t)(b + 1) * lanes;
  double* zw = cl + (size_t)(b + 1) * lanes;
  double* st = zw + (size_t)bw * lanes;
  const size_t ws = (size_t)S * dy;          // doubles of a row of work
  double* w0 = work + (size_t)s * ws + d;
  int si = 0;   // i % bw, kept by hand: a 64-bit remainder per step would cost more than the row
  for (i64 c0 = 0; c0 < T; c0 += MLPG_CHUNK) {
    const int rows = (int)(T - c0 < MLPG_CHUNK ? T - c0 : MLPG_CHUNK);
    mlpg_stage(st, lanes, w0 + (size_t)c0 * ws, dy, rows * S);
    for (int ii = 0; ii < rows; ++ii, si = si + 1 == bw ? 0 : si + 1) {
      const i64 i = c0 + ii;
      double* w = w0 + (size_t)i * ws;
      const double* sr = st + (size_t)ii * S * lanes;
      const int kmax = (int)(i < b ? i : b);
      for (int k = kmax; k >= 1; --k) {
        const double* Lj = Lw + (size_t)mlpg_ring(si - k, bw) * (b + 1) * lanes;
        double v = sr[k * lanes];
        for (int km = kmax; km > k; --km) v = fma(-ct[km * lanes], Lj[(km - k) * lanes], v);
        ct[k * lanes] = v;
        cl[k * lanes] = v / Lj[0];
      }
      double dd = sr[0], z = sr[(S - 1) * lanes];
      for (int k = kmax; k >= 1; --k) {
        dd = fma(-ct[k * lanes], cl[k * lanes], dd);
        z = fma(-cl[k * lanes], zw[mlpg_ring(si - k, bw) * lanes], z);
      }
      double* Li = Lw + (size_t)si * (b + 1) * lanes;
      Li[0] = dd;
      w[0] = dd;
      for (int k = 1; k <= kmax; ++k) {
        const double l = cl[k * lanes];
        Li[k * lanes] = l;
        w[(size_t)k * dy] = l;
      }
      zw[si * lanes] = z;
      w[(size_t)(S - 1) * dy] = z;
    }
  }
  // back: zw[i % bw] collects -sum_k L[i + k][i] y_(i + k) as the rows above are done (row j subtracts L[j][j - k] y_j from
  // the slots of rows j - k: only row j's own entries are needed, so a chunk is staged as in the forward sweep)
  for (int k = 0; k < bw; ++k) zw[k * lanes] = 0.0;
  si = (int)((T - 1) % bw);
  for (i64 c0 = (T - 1) / MLPG_CHUNK * MLPG_CHUNK; c0 >= 0; c0 -= MLPG_CHUNK) {
    const int rows = (int)(T - c0 < MLPG_CHUNK ? T - c0 : MLPG_CHUNK);
    mlpg_stage(st, lanes, w0 + (size_t)c0 * ws, dy, rows * S);
    for (int ii = rows - 1; ii >= 0; --ii, si = si == 0 ? bw - 1 : si - 1) {
      const i64 i = c0 + ii;
      const double* sr = st + (size_t)ii * S * lanes;
      const double y = sr[(S - 1) * lanes] / sr[0] + zw[si * lanes];
      zw[si * lanes] = 0.0;   // the slot is row i - bw's from here on
      const int kmax = (int)(i < b ? i : b);
      for (int k = 1; k <= kmax; ++k) {
        double* p = zw + mlpg_ring(si - k, bw) * lanes;
        *p = fma(-sr[k * lanes], y, *p);
      }
      Y[(size_t)(s + i) * dy + d] = y;
    }
  }
}
}  // namespace eaqhm

using namespace eaqhm;

extern "C" int eaqhm_ceps_delta(eaqhm_ctx* ctx, const double* C, int64_t n, int32_t cols, int32_t span, double* out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!C || !out) return ctx->fail(EAQHM_EINVAL, "eaqhm_ceps_delta: bad argument");
  if (n < 1 || n > MLPG_NMAX || cols < 1 || cols > MLPG_COLS_MAX || span < 1 || span > MLPG_SPAN_MAX)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_ceps_delta: need 1 <= n <= 2^31, 1 <= cols <= 128, 1 <= span <= 8");
  hipLaunchKernelGGL(eaqhm_ceps_delta_kernel, dim3((unsigned)((n * cols + 255) / 256)), dim3(256), 0, ctx->stream, C,
                     (i64)n, (int)cols, (int)span, out);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int64_t eaqhm_mlpg_work_len(int64_t n, int32_t dy, int32_t span) {
  if (!mlpg_sizes_ok(n, dy, span)) return -1;
  return n * mlpg_slots(span) * dy;
}

extern "C" int eaqhm_mlpg_solve(eaqhm_ctx* ctx, const double* P, const double* r, int64_t n, int32_t dy, int32_t span,
                                const int64_t* run_start, const int64_t* run_len, int64_t n_runs, double* work,
                                double* Y) {
  if (!ctx) return EAQHM_EINVAL;
  if (!P || !r || !work || !Y || (n_runs > 0 && (!run_start || !run_len)))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_mlpg_solve: bad argument");
  if (!mlpg_sizes_ok(n, dy, span) || n_runs < 0 || n_runs > n)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_mlpg_solve: need 1 <= n <= 2^31, 1 <= dy <= 64, 1 <= span <= 8, 0 <= n_runs <= n");
  if (n_runs == 0) return EAQHM_OK;
  hipLaunchKernelGGL(eaqhm_mlpg_band_kernel, dim3((unsigned)((n * dy + 255) / 256)), dim3(256), 0, ctx->stream, P, r,
                     (i64)n, (int)dy, (int)span, (const i64*)run_start, (const i64*)run_len, (i64)n_runs, work);
  const int lanes = mlpg_lanes(span);
  const size_t lds = mlpg_lds_doubles(span) * sizeof(double);
  hipLaunchKernelGGL(eaqhm_mlpg_solve_kernel, dim3((unsigned)n_runs, (unsigned)((dy + lanes - 1) / lanes)), dim3(lanes),
                     lds, ctx->stream, (i64)n, (int)dy, (int)span, (const i64*)run_start, (const i64*)run_len, work, Y);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
