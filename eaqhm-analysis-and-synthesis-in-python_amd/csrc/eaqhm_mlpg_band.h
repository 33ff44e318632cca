// eaqhm_mlpg_band.h — what the trajectory solve (eaqhm_mlpg.hip) and the global-variance ascent (eaqhm_gv.hip) share:
// the size limits, the delta rule's coefficients and the lookup of a row's run.  gfx950 only.
#pragma once
#include "eaqhm_common.h"

namespace eaqhm {

typedef long long i64;

constexpr int MLPG_SPAN_MAX = 8;
constexpr int MLPG_DY_MAX = 64;          // static target columns at most
constexpr int MLPG_COLS_MAX = 128;       // columns of the delta builder at most
constexpr i64 MLPG_NMAX = (i64)1 << 31;  // rows at most: n * 128 / 256 blocks stay below 2^31

__host__ __device__ inline int mlpg_slots(int span) { return 2 * span + 2; }   // band entries 0 .. 2 span, then q / z
__host__ __device__ inline double mlpg_denominator(int span) {
  int s = 0;
  for (int k = 1; k <= span; ++k) s += k * k;
  return 2.0 * s;
}

inline bool mlpg_sizes_ok(int64_t n, int32_t dy, int32_t span) {
  return n >= 1 && n <= MLPG_NMAX && dy >= 1 && dy <= MLPG_DY_MAX && span >= 1 && span <= MLPG_SPAN_MAX;
}

// Entry (u, c) of W, the T x T matrix of the delta rule on a run of T rows: sum over tau (ascending) of
// w_tau ([clip(u + tau) = c] - [clip(u - tau) = c]).  It is zero unless |u - c| <= span.
__device__ inline double mlpg_coef(i64 u, i64 c, i64 T, int span, double den) {
  double a = 0.0;
  for (int tau = 1; tau <= span; ++tau) {
    const i64 hi = u + tau < T - 1 ? u + tau : T - 1, lo = u - tau > 0 ? u - tau : 0;
    const double w = (double)tau / den;
    if (hi == c) a += w;
    if (lo == c) a -= w;
  }
  return a;
}

// The run that holds row t (runs disjoint and ascending): -1 when none does or its bounds leave [0, n).
__device__ inline i64 mlpg_find_run(const i64* __restrict__ run_start, const i64* __restrict__ run_len, i64 n_runs, i64 n,
                                    i64 t) {
  i64 lo = 0, hi = n_runs;   // the last run with run_start <= t
  while (lo < hi) {
    const i64 mid = (lo + hi) >> 1;
    if (run_start[mid] <= t) lo = mid + 1; else hi = mid;
  }
  const i64 r = lo - 1;
  if (r < 0) return -1;
  const i64 s = run_start[r], T = run_len[r];
  if (s < 0 || T < 1 || T > n || s > n - T || t >= s + T) return -1;
  return r;
}
}  // namespace eaqhm
