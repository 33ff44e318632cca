// eaqhm_gv.hip — the global-variance term of the trajectory conversion (Toda, Black & Tokuda 2007):
// from the maximum-likelihood trajectory y_ML of eaqhm_mlpg_solve, K Jacobi sweeps up the objective
//   L_d(y) = -(omega / 2)(y^T R y - 2 q^T y) - (1/2) pv_d (v(y) - mu_d)^2,   omega = 1 / (2 N),
// per static column d over all N rows of all runs.  gfx950 (MI355X) only, FP64 on the vector pipe.
//
//   eaqhm_gv_band_kernel     one thread per (row, column): row i of the band of R and q_i into `work` (the arithmetic of
//                            eaqhm_mlpg_band_kernel, with zeros where the band crosses the run's edge), and the row's
//                            distance to its run's edges
//   eaqhm_gv_sum_kernel      per chunk: the sums of y_ML and the number of rows in runs
//   eaqhm_gv_moments_kernel  per (chunk, column): the sums of (y - m)^2, y (R y) and q y
//   eaqhm_gv_start_kernel    the start y^(0) = m + sqrt(mu / v)(y_ML - m), which columns are frozen, L_d(y_ML)
//   eaqhm_gv_step_kernel     trace[k] and one sweep from the old y into the other buffer
//   eaqhm_gv_close_kernel    trace[K], and the copy of the result into Y when it sits in the second buffer
//
// A block is one chunk of eaqhm_gv_chunk_rows(n) rows.  It takes 256 / dy rows a pass, lane -> (row of the pass,
// column): consecutive lanes read consecutive doubles, a lane keeps its column, and the neighbours of row t are at
// +- k dy.  Sums: each lane adds its own rows in ascending order, the lanes of a column are added by a fixed tree in LDS,
// and every block re-adds the per-chunk sums of the launch before in chunk order.  Order between the launches is stream
// order and nothing else: no grid barrier, no flags, no atomics; every word has one writer per launch (words that
// every block would write the same, the trace and the per-column state, are written by block 0), so the same input
// gives the same bits.  No scratch; LDS 3 x 256 + 10 x 64 doubles at most.
#include "eaqhm_mlpg_band.h"

namespace eaqhm {

constexpr int GV_BLOCK = 256;
constexpr i64 GV_CHUNK_MIN = 64;      // rows of a chunk at least, and what their number is a multiple of
constexpr i64 GV_CHUNKS_MAX = 512;    // chunks at most: what every block re-adds per column
constexpr int GV_ITERS_MAX = 10000;

__host__ __device__ inline i64 gv_chunk_rows(i64 n) {
  const i64 per = (n + GV_CHUNKS_MAX - 1) / GV_CHUNKS_MAX;
  return (per + GV_CHUNK_MIN - 1) / GV_CHUNK_MIN * GV_CHUNK_MIN;
}

// `work`, in doubles: the band and q as eaqhm_mlpg_solve lays them out, [n][2 span + 2][dy]; edge [n]; the second
// trajectory buffer [n][dy]; per chunk the sums of y of either buffer, of (y - m)^2, y (R y), q y [chunks][dy] each and
// the number of rows in runs [chunks]; per column the frozen flag and L_d(y_ML) [2][dy]
struct GvLayout {
  i64 chunks;
  size_t edge, yb, sy[2], s2, ry, qy, cnt, col, total;
};
inline GvLayout gv_layout(i64 n, int dy, int span) {
  GvLayout w;
  const i64 rows = gv_chunk_rows(n);
  w.chunks = (n + rows - 1) / rows;
  const size_t per = (size_t)w.chunks * dy;
  w.edge = (size_t)n * mlpg_slots(span) * dy;
  w.yb = w.edge + (size_t)n;
  w.sy[0] = w.yb + (size_t)n * dy;
  w.sy[1] = w.sy[0] + per;
  w.s2 = w.sy[1] + per;
  w.ry = w.s2 + per;
  w.qy = w.ry + per;
  w.cnt = w.qy + per;
  w.col = w.cnt + (size_t)w.chunks;
  w.total = w.col + (size_t)2 * dy;
  return w;
}

// ------------------------------------------------------------------------------------------------
// work[(t S + k) dy + d], S = 2 span + 2: k = 0 .. 2 span holds R[i][i - k] (i the row's index in its run; 0 where
// i - k < 0), k = 2 span + 1 holds q_i.  u ascending in every sum: eaqhm_mlpg_band_kernel's arithmetic, entry by entry.
// edge[t] = lo + 32 hi, lo = min(i, 2 span) and hi = min(T - 1 - i, 2 span) the row's neighbours inside its run on either
// side; -1 for a row that no run holds (its band is not written).
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_gv_band_kernel(const double* __restrict__ P, const double* __restrict__ r, i64 n, int dy, int span,
                         const i64* __restrict__ run_start, const i64* __restrict__ run_len, i64 n_runs,
                         double* __restrict__ work, double* __restrict__ edge) {
  const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * dy) return;
  const i64 t = idx / dy;
  const int d = (int)(idx - t * dy);
  const i64 run = mlpg_find_run(run_start, run_len, n_runs, n, t);
  if (run < 0) {
    if (d == 0) edge[t] = -1.0;
    return;
  }
  const i64 s = run_start[run], T = run_len[run], i = t - s;
  const int S = mlpg_slots(span), b = 2 * span;
  const double den = mlpg_denominator(span);
  const size_t row = (size_t)2 * dy;
  const i64 u0 = i - span > 0 ? i - span : 0;
  double* w = work + (size_t)t * S * dy + d;
  const int lo = (int)(i < b ? i : b), hi = (int)(T - 1 - i < b ? T - 1 - i : b);
  if (d == 0) edge[t] = (double)(lo + 32 * hi);
  for (int k = 0; k <= b; ++k) {
    double acc = 0.0;
    if (k <= lo) {
      const i64 j = i - k, u1 = j + span < T - 1 ? j + span : T - 1;
      if (k == 0) acc = P[(size_t)t * row + d];
      for (i64 u = u0; u <= u1; ++u)
        acc = fma(mlpg_coef(u, i, T, span, den) * mlpg_coef(u, j, T, span, den), P[(size_t)(s + u) * row + dy + d], acc);
    }
    w[(size_t)k * dy] = acc;
  }
  const i64 u1 = i + span < T - 1 ? i + span : T - 1;
  double acc = r[(size_t)t * row + d];
  for (i64 u = u0; u <= u1; ++u) acc = fma(mlpg_coef(u, i, T, span, den), r[(size_t)(s + u) * row + dy + d], acc);
  w[(size_t)(S - 1) * dy] = acc;
}

// ------------------------------------------------------------------------------------------------
// A lane's place in its block's passes: 256 / dy rows a pass, the lanes beyond them idle.
struct GvLane {
  int rpp, rr, d;
  bool on;
};
__device__ inline GvLane gv_lane(int dy) {
  GvLane l;
  l.rpp = GV_BLOCK / dy;
  l.rr = (int)threadIdx.x / dy;
  l.d = (int)threadIdx.x - l.rr * dy;
  l.on = l.rr < l.rpp;
  return l;
}

// The lanes of a column added by a fixed tree: red[j][tid] <- the lane's value, then stride s = 2^k downwards, row rr of
// the pass takes row rr + s.  The sums end in red[j][d].  Every lane of the block calls it.
__device__ inline void gv_reduce(double (*red)[GV_BLOCK], const GvLane& l, int dy, double a0, double a1, double a2) {
  const int tid = threadIdx.x;
  red[0][tid] = a0;
  red[1][tid] = a1;
  red[2][tid] = a2;
  __syncthreads();
  int p2 = 1;
  while (p2 < l.rpp) p2 <<= 1;
  for (int s = p2 >> 1; s >= 1; s >>= 1) {
    if (l.on && l.rr < s && l.rr + s < l.rpp) {
      red[0][tid] += red[0][tid + s * dy];
      red[1][tid] += red[1][tid + s * dy];
      red[2][tid] += red[2][tid + s * dy];
    }
    __syncthreads();
  }
}

// (R y)_t of a row with lo and hi neighbours in its run: the diagonal, the lower band k ascending, the upper band
// (R[t + k][t], row t + k's entry k) k ascending.  band and y point at (t, d).
__device__ inline double gv_Ry(const double* __restrict__ band, const double* __restrict__ y, int dy, int S, int lo,
                               int hi) {
  double acc = band[0] * y[0];
  for (int k = 1; k <= lo; ++k) acc = fma(band[(size_t)k * dy], y[-(i64)k * dy], acc);
  for (int k = 1; k <= hi; ++k) acc = fma(band[((size_t)k * S + k) * dy], y[(i64)k * dy], acc);
  return acc;
}

// The sum over the chunks, ascending.  The loads of 16 chunks are issued together, so the thread waits for the memory
// once per 16 terms, not once per term (one thread adds a column: the order is the point); the additions stay in order.
constexpr int GV_BATCH = 16;
__device__ inline double gv_readd(const double* __restrict__ part, i64 chunks, int stride, int d) {
  double a = 0.0;
  i64 c = 0;
  for (; c + GV_BATCH <= chunks; c += GV_BATCH) {
    double v[GV_BATCH];
#pragma unroll
    for (int u = 0; u < GV_BATCH; ++u) v[u] = part[(size_t)(c + u) * stride + d];
#pragma unroll
    for (int u = 0; u < GV_BATCH; ++u) a += v[u];
  }
  for (; c < chunks; ++c) a += part[(size_t)c * stride + d];
  return a;
}
// The same for a column's sums of y and the numbers of rows at once: m and N.
__device__ inline void gv_readd_mean(const double* __restrict__ sy, const double* __restrict__ cnt, i64 chunks, int dy,
                                     int d, double& m, double& N) {
  double a = 0.0, k = 0.0;
  i64 c = 0;
  for (; c + GV_BATCH <= chunks; c += GV_BATCH) {
    double v[GV_BATCH], w[GV_BATCH];
#pragma unroll
    for (int u = 0; u < GV_BATCH; ++u) {
      v[u] = sy[(size_t)(c + u) * dy + d];
      w[u] = cnt[c + u];
    }
#pragma unroll
    for (int u = 0; u < GV_BATCH; ++u) {
      a += v[u];
      k += w[u];
    }
  }
  for (; c < chunks; ++c) {
    a += sy[(size_t)c * dy + d];
    k += cnt[c];
  }
  N = k;
  m = a / k;
}

// ------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_gv_sum_kernel(const double* __restrict__ Y, const double* __restrict__ edge, i64 n, int dy, i64 chunk_rows,
                        double* __restrict__ sy, double* __restrict__ cnt) {
  __shared__ double red[3][GV_BLOCK];
  const GvLane l = gv_lane(dy);
  const i64 t0 = (i64)blockIdx.x * chunk_rows, t1 = t0 + chunk_rows < n ? t0 + chunk_rows : n;
  double a = 0.0, rows = 0.0;
  if (l.on)
    for (i64 t = t0 + l.rr; t < t1; t += l.rpp) {
      if (edge[t] < 0.0) continue;
      a += Y[(size_t)t * dy + l.d];
      rows += 1.0;
    }
  gv_reduce(red, l, dy, a, rows, 0.0);
  if ((int)threadIdx.x < dy) sy[(size_t)blockIdx.x * dy + threadIdx.x] = red[0][threadIdx.x];
  if (threadIdx.x == 0) cnt[blockIdx.x] = red[1][0];
}

extern "C" __global__ void __launch_bounds__(256)
    eaqhm_gv_moments_kernel(const double* __restrict__ y, const double* __restrict__ work, const double* __restrict__ edge,
                            i64 n, int dy, int span, i64 chunk_rows, i64 chunks, const double* __restrict__ sy,
                            const double* __restrict__ cnt, double* __restrict__ s2, double* __restrict__ ry,
                            double* __restrict__ qy) {
  __shared__ double red[3][GV_BLOCK];
  __shared__ double mean[MLPG_DY_MAX];
  const GvLane l = gv_lane(dy);
  if ((int)threadIdx.x < dy) {
    double N;
    gv_readd_mean(sy, cnt, chunks, dy, threadIdx.x, mean[threadIdx.x], N);
  }
  __syncthreads();
  const int S = mlpg_slots(span);
  const i64 t0 = (i64)blockIdx.x * chunk_rows, t1 = t0 + chunk_rows < n ? t0 + chunk_rows : n;
  double a2 = 0.0, ar = 0.0, aq = 0.0;
  if (l.on) {
    const double m = mean[l.d];
    for (i64 t = t0 + l.rr; t < t1; t += l.rpp) {
      const double e = edge[t];
      if (e < 0.0) continue;
      const int ei = (int)e;
      const double* band = work + (size_t)t * S * dy + l.d;
      const double* yt = y + (size_t)t * dy + l.d;
      const double v = yt[0], dev = v - m;
      a2 = fma(dev, dev, a2);
      ar = fma(v, gv_Ry(band, yt, dy, S, ei & 31, ei >> 5), ar);
      aq = fma(band[(size_t)(S - 1) * dy], v, aq);
    }
  }
  gv_reduce(red, l, dy, a2, ar, aq);
  if ((int)threadIdx.x < dy) {
    const size_t o = (size_t)blockIdx.x * dy + threadIdx.x;
    s2[o] = red[0][threadIdx.x];
    ry[o] = red[1][threadIdx.x];
    qy[o] = red[2][threadIdx.x];
  }
}

// What a block knows of column d once the per-chunk sums are re-added.  Every thread of the block calls it (it holds a
// barrier); the first 4 dy <= 256 of them work: thread a dy + d re-adds array a of column d (y with the row counts,
// (y - m)^2, y (R y), q y) into tot[a][d], then thread d < dy puts them together and is the one that gets the result.
struct GvColumn {
  double N, m, v, L;
};
__device__ inline GvColumn gv_column(double (*tot)[MLPG_DY_MAX], const double* sy, const double* cnt, const double* s2,
                                     const double* ry, const double* qy, i64 chunks, int dy, const double* gv_mean,
                                     const double* gv_prec) {
  const int a = (int)threadIdx.x / dy, d = (int)threadIdx.x - a * dy;
  if (a == 0)
    gv_readd_mean(sy, cnt, chunks, dy, d, tot[0][d], tot[4][d]);
  else if (a < 4)
    tot[a][d] = gv_readd(a == 1 ? s2 : a == 2 ? ry : qy, chunks, dy, d);
  __syncthreads();
  GvColumn c = {0.0, 0.0, 0.0, 0.0};
  if (a == 0) {
    c.N = tot[4][d];
    c.m = tot[0][d];
    c.v = tot[1][d] / c.N;
    const double omega = 1.0 / (2.0 * c.N), dv = c.v - gv_mean[d];
    c.L = -0.5 * omega * (tot[2][d] - 2.0 * tot[3][d]) - 0.5 * gv_prec[d] * dv * dv;
  }
  return c;
}

// Y (y_ML) -> yb (the scaled start; a frozen column's y_ML as it is), the per-chunk sums of yb, and col[0][d] = 1 for a
// frozen column (N < 2 or v(y_ML) = 0), col[1][d] = L_d(y_ML).
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_gv_start_kernel(const double* __restrict__ Y, double* __restrict__ yb, const double* __restrict__ edge, i64 n,
                          int dy, i64 chunk_rows, i64 chunks, const double* __restrict__ sy, const double* __restrict__ cnt,
                          const double* __restrict__ s2, const double* __restrict__ ry, const double* __restrict__ qy,
                          const double* __restrict__ gv_mean, const double* __restrict__ gv_prec,
                          double* __restrict__ sy_new, double* __restrict__ col) {
  __shared__ double red[3][GV_BLOCK];
  __shared__ double tot[5][MLPG_DY_MAX], mean[MLPG_DY_MAX], scale[MLPG_DY_MAX], frozen[MLPG_DY_MAX];
  const GvLane l = gv_lane(dy);
  const GvColumn c = gv_column(tot, sy, cnt, s2, ry, qy, chunks, dy, gv_mean, gv_prec);
  if ((int)threadIdx.x < dy) {
    const int d = threadIdx.x;
    const double mu = gv_mean[d];
    const bool fr = c.N < 2.0 || !(c.v > 0.0);
    mean[d] = c.m;
    scale[d] = fr ? 1.0 : sqrt(mu / c.v);
    frozen[d] = fr ? 1.0 : 0.0;
    if (blockIdx.x == 0) {
      col[d] = fr ? 1.0 : 0.0;
      col[dy + d] = c.L;
    }
  }
  __syncthreads();
  const i64 t0 = (i64)blockIdx.x * chunk_rows, t1 = t0 + chunk_rows < n ? t0 + chunk_rows : n;
  double a = 0.0;
  if (l.on) {
    const double m = mean[l.d], sc = scale[l.d];
    const bool fr = frozen[l.d] != 0.0;
    for (i64 t = t0 + l.rr; t < t1; t += l.rpp) {
      if (edge[t] < 0.0) continue;
      const double v = Y[(size_t)t * dy + l.d], out = fr ? v : fma(sc, v - m, m);
      yb[(size_t)t * dy + l.d] = out;
      a += out;
    }
  }
  gv_reduce(red, l, dy, a, 0.0, 0.0);
  if ((int)threadIdx.x < dy) sy_new[(size_t)blockIdx.x * dy + threadIdx.x] = red[0][threadIdx.x];
}

// trace_k[d] = L_d(y) (a frozen column: L_d(y_ML)) when trace_k is given, then y_new = y + g / h (a frozen column: y),
// g = omega (q - R y) - pv (v - mu)(2 / N)(y - m), h = (4 span + 1) omega R_tt + pv (2 / N)(|v - mu| + 2 v), and the
// per-chunk sums of y_new.
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_gv_step_kernel(const double* __restrict__ y, double* __restrict__ y_new, const double* __restrict__ work,
                         const double* __restrict__ edge, i64 n, int dy, int span, i64 chunk_rows, i64 chunks,
                         const double* __restrict__ sy, const double* __restrict__ cnt, const double* __restrict__ s2,
                         const double* __restrict__ ry, const double* __restrict__ qy, const double* __restrict__ gv_mean,
                         const double* __restrict__ gv_prec, const double* __restrict__ col, double* __restrict__ sy_new,
                         double* __restrict__ trace_k) {
  __shared__ double red[3][GV_BLOCK];
  __shared__ double tot[5][MLPG_DY_MAX], mean[MLPG_DY_MAX], pull[MLPG_DY_MAX], curv[MLPG_DY_MAX], frozen[MLPG_DY_MAX],
      omega_s[MLPG_DY_MAX];
  const GvLane l = gv_lane(dy);
  const GvColumn c = gv_column(tot, sy, cnt, s2, ry, qy, chunks, dy, gv_mean, gv_prec);
  if ((int)threadIdx.x < dy) {
    const int d = threadIdx.x;
    const double mu = gv_mean[d], pv = gv_prec[d];
    const bool fr = col[d] != 0.0;
    const double dv = c.v - mu, two_n = 2.0 / c.N;
    mean[d] = c.m;
    pull[d] = pv * dv * two_n;
    curv[d] = pv * two_n * (fabs(dv) + 2.0 * c.v);
    frozen[d] = fr ? 1.0 : 0.0;
    omega_s[d] = 1.0 / (2.0 * c.N);
    if (blockIdx.x == 0 && trace_k) trace_k[d] = fr ? col[dy + d] : c.L;
  }
  __syncthreads();
  const int S = mlpg_slots(span);
  const double maj = (double)(4 * span + 1);
  const i64 t0 = (i64)blockIdx.x * chunk_rows, t1 = t0 + chunk_rows < n ? t0 + chunk_rows : n;
  double a = 0.0;
  if (l.on) {
    const double m = mean[l.d], pl = pull[l.d], cv = curv[l.d], omega = omega_s[l.d];
    const bool fr = frozen[l.d] != 0.0;
    for (i64 t = t0 + l.rr; t < t1; t += l.rpp) {
      const double e = edge[t];
      if (e < 0.0) continue;
      const double* yt = y + (size_t)t * dy + l.d;
      double out = yt[0];
      if (!fr) {
        const int ei = (int)e;
        const double* band = work + (size_t)t * S * dy + l.d;
        const double g = omega * (band[(size_t)(S - 1) * dy] - gv_Ry(band, yt, dy, S, ei & 31, ei >> 5)) - pl * (out - m);
        const double h = fma(maj * omega, band[0], cv);
        out += g / h;
      }
      y_new[(size_t)t * dy + l.d] = out;
      a += out;
    }
  }
  gv_reduce(red, l, dy, a, 0.0, 0.0);
  if ((int)threadIdx.x < dy) sy_new[(size_t)blockIdx.x * dy + threadIdx.x] = red[0][threadIdx.x];
}

// The closing launch.  With trace_k (block 0 alone works): trace_k[d] = L_d(y) from the sums of the moments launch before
// (a frozen column: L_d(y_ML)).  With Y: the rows in runs of the second buffer go home into Y.
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_gv_close_kernel(const double* __restrict__ yb, double* __restrict__ Y, const double* __restrict__ edge, i64 n,
                          int dy, i64 chunk_rows, i64 chunks, const double* __restrict__ sy, const double* __restrict__ cnt,
                          const double* __restrict__ s2, const double* __restrict__ ry, const double* __restrict__ qy,
                          const double* __restrict__ gv_mean, const double* __restrict__ gv_prec,
                          const double* __restrict__ col, double* __restrict__ trace_k) {
  __shared__ double tot[5][MLPG_DY_MAX];
  if (trace_k && blockIdx.x == 0) {
    const GvColumn c = gv_column(tot, sy, cnt, s2, ry, qy, chunks, dy, gv_mean, gv_prec);
    if ((int)threadIdx.x < dy) trace_k[threadIdx.x] = col[threadIdx.x] != 0.0 ? col[dy + threadIdx.x] : c.L;
  }
  if (!Y) return;
  const GvLane l = gv_lane(dy);
  const i64 t0 = (i64)blockIdx.x * chunk_rows, t1 = t0 + chunk_rows < n ? t0 + chunk_rows : n;
  if (l.on)
    for (i64 t = t0 + l.rr; t < t1; t += l.rpp)
      if (edge[t] >= 0.0) Y[(size_t)t * dy + l.d] = yb[(size_t)t * dy + l.d];
}
}  // namespace eaqhm

using namespace eaqhm;

extern "C" int64_t eaqhm_gv_chunk_rows(int64_t n) { return n >= 1 && n <= MLPG_NMAX ? gv_chunk_rows(n) : -1; }

extern "C" int64_t eaqhm_gv_work_len(int64_t n, int32_t dy, int32_t span) {
  if (!mlpg_sizes_ok(n, dy, span)) return -1;
  return (int64_t)gv_layout(n, dy, span).total;
}

extern "C" int eaqhm_gv_ascend(eaqhm_ctx* ctx, const double* P, const double* r, int64_t n, int32_t dy, int32_t span,
                               const int64_t* run_start, const int64_t* run_len, int64_t n_runs, const double* gv_mean,
                               const double* gv_prec, int32_t iters, double* work, double* Y, double* trace) {
  if (!ctx) return EAQHM_EINVAL;
  if (!P || !r || !gv_mean || !gv_prec || !work || !Y || (n_runs > 0 && (!run_start || !run_len)))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_gv_ascend: bad argument");
  if (!mlpg_sizes_ok(n, dy, span) || n_runs < 0 || n_runs > n || iters < 0 || iters > GV_ITERS_MAX)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_gv_ascend: need 1 <= n <= 2^31, 1 <= dy <= 64, 1 <= span <= 8, 0 <= n_runs <= n, "
                                   "0 <= iters <= 10000");
  if (n_runs == 0) return EAQHM_OK;
  const GvLayout w = gv_layout(n, dy, span);
  const i64 rows = gv_chunk_rows(n);
  const dim3 grid((unsigned)w.chunks), block(GV_BLOCK);
  double *edge = work + w.edge, *sy[2] = {work + w.sy[0], work + w.sy[1]}, *s2 = work + w.s2, *ry = work + w.ry,
         *qy = work + w.qy, *cnt = work + w.cnt, *col = work + w.col;
  double* buf[2] = {Y, work + w.yb};
  hipLaunchKernelGGL(eaqhm_gv_band_kernel, dim3((unsigned)((n * dy + 255) / 256)), block, 0, ctx->stream, P, r, (i64)n,
                     (int)dy, (int)span, (const i64*)run_start, (const i64*)run_len, (i64)n_runs, work, edge);
  hipLaunchKernelGGL(eaqhm_gv_sum_kernel, grid, block, 0, ctx->stream, (const double*)Y, (const double*)edge, (i64)n,
                     (int)dy, rows, sy[0], cnt);
  auto moments = [&](int cur) {   // of buf[cur], whose per-chunk sums of y are sy[cur]
    hipLaunchKernelGGL(eaqhm_gv_moments_kernel, grid, block, 0, ctx->stream, (const double*)buf[cur], (const double*)work,
                       (const double*)edge, (i64)n, (int)dy, (int)span, rows, w.chunks, (const double*)sy[cur],
                       (const double*)cnt, s2, ry, qy);
  };
  moments(0);
  hipLaunchKernelGGL(eaqhm_gv_start_kernel, grid, block, 0, ctx->stream, (const double*)Y, buf[1], (const double*)edge,
                     (i64)n, (int)dy, rows, w.chunks, (const double*)sy[0], (const double*)cnt, (const double*)s2,
                     (const double*)ry, (const double*)qy, gv_mean, gv_prec, sy[1], col);
  int cur = 1;
  for (int k = 0; k < iters; ++k, cur = 1 - cur) {
    moments(cur);
    hipLaunchKernelGGL(eaqhm_gv_step_kernel, grid, block, 0, ctx->stream, (const double*)buf[cur], buf[1 - cur],
                       (const double*)work, (const double*)edge, (i64)n, (int)dy, (int)span, rows, w.chunks,
                       (const double*)sy[cur], (const double*)cnt, (const double*)s2, (const double*)ry, (const double*)qy,
                       gv_mean, gv_prec, (const double*)col, sy[1 - cur], trace ? trace + (size_t)k * dy : nullptr);
  }
  if (trace || cur == 1) {   // trace[iters], and the result home when it sits in the second buffer
    if (trace) moments(cur);
    hipLaunchKernelGGL(eaqhm_gv_close_kernel, cur == 1 ? grid : dim3(1), block, 0, ctx->stream, (const double*)buf[1],
                       cur == 1 ? Y : nullptr, (const double*)edge, (i64)n, (int)dy, rows, w.chunks, (const double*)sy[cur],
                       (const double*)cnt, (const double*)s2, (const double*)ry, (const double*)qy, gv_mean, gv_prec,
                       (const double*)col, trace ? trace + (size_t)iters * dy : nullptr);
  }
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
