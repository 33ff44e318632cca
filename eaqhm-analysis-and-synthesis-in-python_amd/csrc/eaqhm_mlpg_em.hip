// eaqhm_mlpg_em.hip — the conditional E-step of the trajectory refinement: the posteriors of the
// mixture's components given the source rows AND the current trajectory.  gfx950 (MI355X) only, FP64 on the matrix pipe
// (v_mfma_f64_16x16x4_f64).
//
//   eaqhm_mlpg_estep_kernel   64 rows per block: Yd = [y | delta y] from the trajectory (the delta over the row's own run),
//                             then per component t = X A_m^T on the matrix pipe, q = sum_j py_mj (Yd_j - t_j - bq_mj)^2,
//                             lp = ln prior + kc_m - q / 2, and the log-sum-exp and the posteriors, one launch
//
// The kernel is eaqhm_gmm_regress_kernel's contraction followed by eaqhm_gmm_estep_kernel's tail (eaqhm_gmm.hip); the
// tile, the stride rules and the 16-lane sum are theirs (eaqhm_gmm_mfma.h).  The delta is eaqhm_ceps_delta_kernel's
// (eaqhm_mlpg.hip): tau ascending, the index clipped to the row's own run, which is found by bisection in run_start as
// eaqhm_mlpg_band_kernel finds it.  Every MFMA operand comes from LDS, where rows and columns beyond the data are zeros.
// No atomics, every word has one writer, the order of every sum is fixed, and a row's result does not depend on where
// the row lies in its block: the same bits on every launch and wherever the run lies in the array.
#include "eaqhm_gmm_mfma.h"
#include "eaqhm_mlpg_band.h"

namespace eaqhm {

constexpr int EM_DX_MAX = 64;    // dynamic source columns at most
constexpr int EM_DY_MAX = 32;    // static target columns at most: 64 with their deltas, four panels of 16
constexpr int EM_M_MAX = 64;     // components at most

// LDS, in doubles from the start:
//   Xs[64][LS]          the block's source rows, LS = gmm_stride_rowk(dx)
//   As[dyp][LS]         A_m, dyp = 2 dy padded to 16; before the first component the same words hold
//   Yh[64 + 2 span][dy]   the trajectory's rows n0 - span .. n0 + 63 + span (zeros outside [0, n))
//   bs[dyp], ps[dyp]    bq_m and py_m
//   Yd[64][LY]          [y | delta y], LY = gmm_stride_krow(dyp)
//   lp[64][M | 1]       ln prior, then lp, then e = exp(lp - max)
//   srow[64]            sum of e: 0 marks a lost row, -1 a row outside every run
//   rs[64], rT[64]      (as int64) the start and the length of each row's run, length 0 outside every run
// At dx = 64, dy = 32, M = 64, span = 8: 144 384 bytes; at dx = 48, dy = 24, M = 8: 90 624 bytes (span 2).  One block per CU.
struct em_layout {
  int dxp, dyp, LS, LY, LM, a_words;
  size_t xs, as, bs, ps, yd, lp, srow, runs, words;
};

__host__ __device__ inline em_layout em_lds(int dx, int dy, int M, int span) {
  em_layout L;
  L.dxp = (dx + 3) & ~3;
  L.dyp = gmm_pad16(2 * dy);
  L.LS = gmm_stride_rowk(dx);
  L.LY = gmm_stride_krow(L.dyp);
  L.LM = M | 1;
  const int halo = (GMM_ROWS + 2 * span) * dy;
  L.a_words = L.dyp * L.LS > halo ? L.dyp * L.LS : halo;
  L.xs = 0;
  L.as = L.xs + (size_t)GMM_ROWS * L.LS;
  L.bs = L.as + L.a_words;
  L.ps = L.bs + L.dyp;
  L.yd = L.ps + L.dyp;
  L.lp = L.yd + (size_t)GMM_ROWS * L.LY;
  L.srow = L.lp + (size_t)GMM_ROWS * L.LM;
  L.runs = L.srow + GMM_ROWS;
  L.words = L.runs + 2 * GMM_ROWS;
  return L;
}

extern "C" __global__ void __launch_bounds__(256)
    eaqhm_mlpg_estep_kernel(const double* __restrict__ X, const double* __restrict__ prior, const double* __restrict__ A,
                            const double* __restrict__ bq, const double* __restrict__ py, const double* __restrict__ kc,
                            const double* __restrict__ Y, i64 n, int dx, int dy, int M, int span,
                            const i64* __restrict__ run_start, const i64* __restrict__ run_len, i64 n_runs,
                            double* __restrict__ gamma, double* __restrict__ ll) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const em_layout L = em_lds(dx, dy, M, span);
  const int dxp = L.dxp, dyp = L.dyp, njp = dyp / 16, LS = L.LS, LY = L.LY, LM = L.LM, dy2 = 2 * dy;
  double* Xs = lds + L.xs;
  double* As = lds + L.as;
  double* Yh = As;
  double* bs = lds + L.bs;
  double* ps = lds + L.ps;
  double* Yd = lds + L.yd;
  double* lp = lds + L.lp;
  double* srow = lds + L.srow;
  i64* rs = (i64*)(lds + L.runs);
  i64* rT = rs + GMM_ROWS;
  const i64 n0 = (i64)blockIdx.x * GMM_ROWS;
  const int rows = (int)(n - n0 < GMM_ROWS ? n - n0 : GMM_ROWS);
  for (int k = tid; k < GMM_ROWS * dxp; k += 256) {
    const int r = k / dxp, j = k - r * dxp;
    Xs[r * LS + j] = r < rows && j < dx ? X[(size_t)(n0 + r) * dx + j] : 0.0;
  }
  for (int k = tid; k < GMM_ROWS * M; k += 256) {
    const int r = k / M, m = k - r * M;
    lp[r * LM + m] = r < rows ? log(prior[(size_t)n0 * M + k]) : 0.0;
  }
  for (int k = tid; k < (GMM_ROWS + 2 * span) * dy; k += 256) {
    const int hr = k / dy, j = k - hr * dy;
    const i64 g = n0 - span + hr;
    Yh[k] = g >= 0 && g < n ? Y[(size_t)g * dy + j] : 0.0;
  }
  if (tid < GMM_ROWS) {
    const i64 run = tid < rows ? mlpg_find_run(run_start, run_len, n_runs, n, n0 + tid) : -1;
    rs[tid] = run < 0 ? 0 : run_start[run];
    rT[tid] = run < 0 ? 0 : run_len[run];
  }
  __syncthreads();
  {   // Yd: the static half is the row itself, the delta half eaqhm_ceps_delta_kernel's sum over the row's own run
    const double den = mlpg_denominator(span);
    const i64 base = n0 - span;
    for (int k = tid; k < GMM_ROWS * dyp; k += 256) {
      const int r = k / dyp, j = k - r * dyp;
      double v = 0.0;
      const i64 T = rT[r];
      if (T > 0 && j < dy2) {
        const i64 t = n0 + r;
        if (j < dy) {
          v = Yh[(int)(t - base) * dy + j];
        } else {
          const i64 lo = rs[r], hi = lo + T - 1;
          const int c = j - dy;
          for (int tau = 1; tau <= span; ++tau) {
            const i64 tp = t + tau < hi ? t + tau : hi, tm = t - tau > lo ? t - tau : lo;
            v = fma((double)tau / den, Yh[(int)(tp - base) * dy + c] - Yh[(int)(tm - base) * dy + c], v);
          }
        }
      }
      Yd[r * LY + j] = v;
    }
  }
  const double* xr = Xs + (16 * w + lr) * LS + lq;
  for (int m = 0; m < M; ++m) {
    __syncthreads();   // Yd is built and Yh read (m = 0); the last component's As, bs and ps are read
    for (int k = tid; k < dyp * dxp; k += 256) {
      const int r = k / dxp, j = k - r * dxp;
      As[r * LS + j] = r < dy2 && j < dx ? A[((size_t)m * dy2 + r) * dx + j] : 0.0;
    }
    for (int j = tid; j < dyp; j += 256) {
      bs[j] = j < dy2 ? bq[(size_t)m * dy2 + j] : 0.0;
      ps[j] = j < dy2 ? py[(size_t)m * dy2 + j] : 0.0;
    }
    __syncthreads();
    double q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int jp = 0; jp < 4; ++jp)
      if (jp < njp) {
        gd4 t = {0.0, 0.0, 0.0, 0.0};
        const double* ar = As + (16 * jp + lr) * LS + lq;
        for (int k0 = 0; k0 < dxp; k0 += 4) t = gmm_mfma(xr[k0], ar[k0], t);
        const double bj = bs[16 * jp + lr], pj = ps[16 * jp + lr];
        for (int r = 0; r < 4; ++r) {
          const double d = Yd[(16 * w + lq + 4 * r) * LY + 16 * jp + lr] - (t[r] + bj);
          q[r] = fma(pj * d, d, q[r]);
        }
      }
    const double km = kc[m];
    for (int r = 0; r < 4; ++r) {
      const double qs = gmm_sum16(q[r]);
      double* p = lp + (16 * w + lq + 4 * r) * LM + m;
      if (lr == 0) *p = (*p + km) - 0.5 * qs;
    }
  }
  __syncthreads();
  if (tid < GMM_ROWS) {   // one lane per row: the largest lp, e = exp(lp - max) in place, their sum
    double s = -1.0;
    if (rT[tid] > 0) {
      double* p = lp + tid * LM;
      double mx = p[0];   // a component with prior 0 has lp = -inf: it does not win the maximum and its e is exactly 0
      for (int m = 1; m < M; ++m) mx = fmax(mx, p[m]);
      // every remaining q overflowed: lp = max = -inf, and -inf - -inf is NaN.  Such a row has ll = -inf and the
      // trajectory expresses no preference: gamma = prior (the last loop copies it)
      const bool lost = mx == -INFINITY;
      s = 0.0;
      if (!lost)
        for (int m = 0; m < M; ++m) {
          const double e = exp(p[m] - mx);
          p[m] = e;
          s += e;
        }
      ll[n0 + tid] = lost ? -INFINITY : mx + log(s);
    }
    srow[tid] = s;
  }
  __syncthreads();
  for (int k = tid; k < rows * M; k += 256) {   // gamma = e / s: a row sums to 1 within the roundings of the quotients
    const int r = k / M, m = k - r * M;
    const double s = srow[r];
    if (s < 0.0) continue;   // outside every run: not written
    gamma[(size_t)n0 * M + k] = s == 0.0 ? prior[(size_t)n0 * M + k] : lp[r * LM + m] / s;
  }
}
}  // namespace eaqhm

using namespace eaqhm;

extern "C" int eaqhm_mlpg_estep(eaqhm_ctx* ctx, const double* X, const double* prior, const double* A, const double* bq,
                                const double* py, const double* kc, const double* Y, int64_t n, int32_t dx, int32_t dy,
                                int32_t M, int32_t span, const int64_t* run_start, const int64_t* run_len, int64_t n_runs,
                                double* gamma_out, double* ll_out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!X || !prior || !A || !bq || !py || !kc || !Y || !gamma_out || !ll_out || (n_runs > 0 && (!run_start || !run_len)))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_mlpg_estep: bad argument");
  if (n < 1 || n > MLPG_NMAX || dx < 1 || dx > EM_DX_MAX || dy < 1 || dy > EM_DY_MAX || M < 1 || M > EM_M_MAX ||
      span < 1 || span > MLPG_SPAN_MAX || n_runs < 0 || n_runs > n)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_mlpg_estep: need 1 <= n <= 2^31, 1 <= dx <= 64, 1 <= dy <= 32, 1 <= M <= 64, "
                                   "1 <= span <= 8, 0 <= n_runs <= n");
  if (n_runs == 0) return EAQHM_OK;
  const size_t lds = em_lds(dx, dy, M, span).words * sizeof(double);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_mlpg_estep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  hipLaunchKernelGGL(eaqhm_mlpg_estep_kernel, dim3((unsigned)((n + GMM_ROWS - 1) / GMM_ROWS)), dim3(256), lds,
                     ctx->stream, X, prior, A, bq, py, kc, Y, (i64)n, (int)dx, (int)dy, (int)M, (int)span,
                     (const i64*)run_start, (const i64*)run_len, (i64)n_runs, gamma_out, ll_out);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
