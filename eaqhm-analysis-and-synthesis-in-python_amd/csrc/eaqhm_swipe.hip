// eaqhm_swipe.hip — the SWIPE' pitch estimator's three stages on the device.  gfx950 (MI355X) only.
//
//   eaqhm_swipe_loudness_kernel<G>  a group of G threads owns one frame: window, in-place complex FFT in LDS (imaginary
//                                   part zero), one-sided density at the two bins around every ERB point, SciPy's linear
//                                   interpolation, sqrt(max(0, .)), the row's 2-norm in a fixed order, the division.
//                                   G = 256 (a block) for w > 256, G = 64 (a wave, four frames a block) below.
//   eaqhm_swipe_scores_kernel       Si = K . L^T on v_mfma_f64_16x16x4_f64 (the lane maps of eaqhm_gmm_mfma.h): a block
//                                   owns 64 candidates x 64 frames, wave w the candidates 16 w .. 16 w + 15; k in chunks of
//                                   32 through LDS, ascending, one accumulator per output.
//   eaqhm_swipe_pick_kernel         a wave owns one instant: the time interpolation of every window's scores, the weighted
//                                   sum per candidate, the first maximum, the quadratic through its neighbours on the
//                                   candidate's fine grid; the pitch is read from the host's table.
//
// The host's NumPy code rounds every operation once, so nothing here may be contracted into an fma: the decisions (which
// candidate, which fine-grid point) are compared with the host's.  No atomics: every output word has one writer.
#include "eaqhm_gmm_mfma.h"
#include "eaqhm_wave.h"
#include "../../include/eaqhm_swipe.h"

#pragma clang fp contract(off)

namespace eaqhm {

typedef long long i64;

constexpr int SW_TILE = 64;   // candidates and frames of a scores block
constexpr int SW_KC = 32;     // columns of a staged chunk

// LDS index of FFT element i: one double of padding after every 32, so that the late stages (four operands a butterfly
// 1, 2, 4 .. apart) spread over the banks.
__device__ inline int sw_at(int i) { return i + (i >> 5); }
__host__ __device__ inline int sw_padded(int w) { return w + (w >> 5); }
// doubles of one group's LDS region: re, im, the row's values, the reduction
__host__ __device__ inline int sw_region(int w, int nE, int G) { return 2 * sw_padded(w) + nE + G; }

// One-sided density at bin k (matplotlib's specgram as swipe.py restates it): X_k sits at the bit-reversed position.
__device__ inline double sw_density(const double* re, const double* im, int k, int w, int logw, double fs, double sumw2) {
  const int at = sw_at((int)(__brev((unsigned)k) >> (32 - logw)));
  const double a = re[at], b = im[at];
  double P = a * a + b * b;
  if (k != 0 && k != (w >> 1)) P *= 2.0;
  P /= fs;
  P /= sumw2;
  return P;
}

template <int G>
__global__ void __launch_bounds__(256)
    eaqhm_swipe_loudness_kernel(const double* __restrict__ x, i64 n, int w, int logw, int hop, i64 pad, i64 nframes,
                                const double* __restrict__ window, double fs, double sumw2, const int* __restrict__ lo,
                                const double* __restrict__ xlo, const double* __restrict__ df, int nE,
                                double* __restrict__ L, i64 ld) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int FPB = 256 / G;   // frames of a block
  const int g = threadIdx.x / G, gt = threadIdx.x % G;
  const int wp = sw_padded(w);
  double* re = lds + (size_t)g * sw_region(w, nE, G);
  double* im = re + wp;
  double* lv = im + wp;
  double* red = lv + nE;
  const i64 m = (i64)blockIdx.x * FPB + g;
  const bool live = m < nframes;   // a group beyond the last frame transforms zeros and writes nothing
  const i64 start = m * hop - pad;
  for (int i = gt; i < w; i += G) {
    const i64 at = start + i;
    re[sw_at(i)] = live && at >= 0 && at < n ? x[at] * window[i] : 0.0;
    im[sw_at(i)] = 0.0;
  }
  __syncthreads();
  // decimation in frequency, in place: a radix-4 stage is two radix-2 stages fused, so the result is in bit-reversed order
  int B = w;
  for (; B >= 4; B >>= 2) {
    const int q = B >> 2;
    for (int b = gt; b < (w >> 2); b += G) {
      const int j = b & (q - 1), i0 = ((b - j) << 2) + j;
      const int p0 = sw_at(i0), p1 = sw_at(i0 + q), p2 = sw_at(i0 + 2 * q), p3 = sw_at(i0 + 3 * q);
      const double a0r = re[p0], a0i = im[p0], a1r = re[p1], a1i = im[p1];
      const double a2r = re[p2], a2i = im[p2], a3r = re[p3], a3i = im[p3];
      const double t0r = a0r + a2r, t0i = a0i + a2i, t1r = a1r + a3r, t1i = a1i + a3i;
      const double t2r = a0r - a2r, t2i = a0i - a2i, t3r = a1r - a3r, t3i = a1i - a3i;
      const double ur = t2r + t3i, ui = t2i - t3r;   // t2 - i t3
      const double vr = t2r - t3i, vi = t2i + t3r;   // t2 + i t3
      const double dr = t0r - t1r, di = t0i - t1i;
      // exp(-2 pi i m j / B), m = 1, 2, 3: the arguments j / (2 q) .. are exact
      double s1, c1, s2, c2, s3, c3;
      const double ang = -(double)j / (double)(2 * q);
      sincospi(ang, &s1, &c1);
      sincospi(2.0 * ang, &s2, &c2);
      sincospi(3.0 * ang, &s3, &c3);
      re[p0] = t0r + t1r;
      im[p0] = t0i + t1i;
      re[p1] = dr * c2 - di * s2;
      im[p1] = dr * s2 + di * c2;
      re[p2] = ur * c1 - ui * s1;
      im[p2] = ur * s1 + ui * c1;
      re[p3] = vr * c3 - vi * s3;
      im[p3] = vr * s3 + vi * c3;
    }
    __syncthreads();
  }
  if (B == 2) {
    for (int b = gt; b < (w >> 1); b += G) {
      const int p0 = sw_at(2 * b), p1 = sw_at(2 * b + 1);
      const double a0r = re[p0], a0i = im[p0], a1r = re[p1], a1i = im[p1];
      re[p0] = a0r + a1r;
      im[p0] = a0i + a1i;
      re[p1] = a0r - a1r;
      im[p1] = a0i - a1i;
    }
    __syncthreads();
  }
  double part = 0.0;
  for (int e = gt; e < nE; e += G) {
    int k = lo[e];
    k = k < 0 ? 0 : (k > (w >> 1) - 1 ? (w >> 1) - 1 : k);
    const double P0 = sw_density(re, im, k, w, logw, fs, sumw2), P1 = sw_density(re, im, k + 1, w, logw, fs, sumw2);
    const double slope = (P1 - P0) / df[e];
    const double v = slope * xlo[e] + P0;
    const double l = sqrt(v > 0.0 ? v : 0.0);
    lv[e] = l;
    part = part + l * l;
  }
  red[gt] = part;
  __syncthreads();
  for (int s = G >> 1; s > 0; s >>= 1) {   // the same tree on every launch
    if (gt < s) red[gt] = red[gt] + red[gt + s];
    __syncthreads();
  }
  const double nrm = sqrt(red[0]);
  if (live) {
    double* row = L + (size_t)m * ld;
    for (int e = gt; e < nE; e += G) row[e] = nrm == 0.0 ? 0.0 : lv[e] / nrm;
  }
}

// Stages rows row0 .. row0 + 63, columns k0 .. k0 + 31 of X [rows][ld] into dst[64][LS]; zeros beyond `rows` and `cols`.
__device__ inline void sw_stage(double* __restrict__ dst, const double* __restrict__ X, i64 row0, i64 rows, i64 ld, int k0,
                                int cols, int LS, int tid) {
  const int c = tid & (SW_KC - 1), r0 = tid >> 5;
  double v[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const i64 r = row0 + r0 + 8 * u;
    v[u] = r < rows && k0 + c < cols ? X[(size_t)r * ld + k0 + c] : 0.0;
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) dst[(r0 + 8 * u) * LS + c] = v[u];
}

// blockIdx.x: 64 frames; blockIdx.y: 64 candidates.
extern "C" __global__ void __launch_bounds__(256)
    eaqhm_swipe_scores_kernel(const double* __restrict__ K, int cand, i64 ldk, const double* __restrict__ L, i64 nframes,
                              i64 ldl, int nE, double* __restrict__ Si) {
  constexpr int LS = SW_KC + 2;   // gmm_stride_rowk(32)
  __shared__ __attribute__((aligned(16))) double Ks[SW_TILE * LS];
  __shared__ __attribute__((aligned(16))) double Ls[SW_TILE * LS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const i64 f0 = (i64)blockIdx.x * SW_TILE;
  const int c0 = blockIdx.y * SW_TILE;
  gd4 t0 = {0.0, 0.0, 0.0, 0.0}, t1 = t0, t2 = t0, t3 = t0;
  const double* ar = Ks + (16 * w + lr) * LS + lq;
  const double* br = Ls + lr * LS + lq;
  for (int k0 = 0; k0 < nE; k0 += SW_KC) {
    __syncthreads();   // the last chunk is read
    sw_stage(Ks, K, c0, cand, ldk, k0, nE, LS, tid);
    sw_stage(Ls, L, f0, nframes, ldl, k0, nE, LS, tid);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SW_KC; k += 4) {
      const double a = ar[k];
      t0 = gmm_mfma(a, br[k], t0);
      t1 = gmm_mfma(a, br[16 * LS + k], t1);
      t2 = gmm_mfma(a, br[32 * LS + k], t2);
      t3 = gmm_mfma(a, br[48 * LS + k], t3);
    }
  }
  const gd4 t[4] = {t0, t1, t2, t3};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const i64 f = f0 + 16 * c + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = c0 + 16 * w + lq + 4 * r;
      if (i < cand && f < nframes) Si[(size_t)i * nframes + f] = t[c][r];
    }
  }
}

struct SwipeWin {
  const double* Si;   // [nc][nfr]
  const double* mu;   // [nc]
  const double* ts;   // [nfr]
  i64 nfr;
  int j0, nc;
};
struct SwipeWins {
  SwipeWin win[EAQHM_SWIPE_WINDOWS];
};

// S of candidate c at the wave's instant: the windows in index order, from an exact 0 as swipe.py's S does.
__device__ inline double sw_strength(int c, int nwin, const SwipeWin* wins, const i64* lo, const double* dt,
                                     const double* dts) {
  double acc = 0.0;
  for (int v = 0; v < nwin; ++v) {
    const int r = c - wins[v].j0;
    if (r < 0 || r >= wins[v].nc) continue;
    const double* row = wins[v].Si + (size_t)r * wins[v].nfr + lo[v];
    const double y0 = row[0], y1 = row[1];
    const double slope = (y1 - y0) / dts[v];
    const double y = slope * dt[v] + y0;
    acc = acc + wins[v].mu[r] * y;
  }
  return acc;
}

extern "C" __global__ void __launch_bounds__(256)
    eaqhm_swipe_pick_kernel(SwipeWins a, int nwin, const double* __restrict__ t, i64 T, int npc, double pc0,
                            const double* __restrict__ ntc, const double* __restrict__ nftc,
                            const double* __restrict__ ptab, const int* __restrict__ nf, int nfmax,
                            double* __restrict__ p, double* __restrict__ s, double* __restrict__ S) {
  __shared__ SwipeWin wins[EAQHM_SWIPE_WINDOWS];
  __shared__ i64 lo_s[4][EAQHM_SWIPE_WINDOWS];
  __shared__ double dt_s[4][EAQHM_SWIPE_WINDOWS], dts_s[4][EAQHM_SWIPE_WINDOWS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 0; v < EAQHM_SWIPE_WINDOWS; ++v) wins[v] = a.win[v];
  }
  __syncthreads();
  const i64 it = (i64)blockIdx.x * 4 + wv;
  const bool live = it < T;   // a wave beyond the last instant works on the last one and writes nothing
  const double tv = t[live ? it : T - 1];
  if (lane < nwin) {   // numpy.searchsorted(ts, tv) clipped to [1, nfr - 1]: SciPy's interval
    const double* ts = wins[lane].ts;
    i64 b = 0, e = wins[lane].nfr;
    while (b < e) {
      const i64 mid = (b + e) >> 1;
      if (ts[mid] < tv) b = mid + 1;
      else e = mid;
    }
    const i64 hi = b < 1 ? 1 : (b > wins[lane].nfr - 1 ? wins[lane].nfr - 1 : b);
    lo_s[wv][lane] = hi - 1;
    dt_s[wv][lane] = tv - ts[hi - 1];
    dts_s[wv][lane] = ts[hi] - ts[hi - 1];
  }
  __syncthreads();
  const i64* lo = lo_s[wv];
  const double *dt = dt_s[wv], *dts = dts_s[wv];
  double bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < npc; c += 64) {   // ascending per lane: a later candidate wins only with a larger value
    const double v = sw_strength(c, nwin, wins, lo, dt, dts);
    if (S && live) S[(size_t)c * T + it] = v;
    if (c == lane || v > bv) {
      bv = v;
      bi = c;
    }
  }
  wave_first_max(bv, bi);
  if (bi == 0 || bi == npc - 1) {   // swipe.py: a maximum on either edge maps to the first candidate
    if (live && lane == 0) {
      p[it] = pc0;
      s[it] = bv;
    }
    return;
  }
  // the quadratic through the three neighbours, Newton's form turned into c2 x^2 + c1 x + c0
  const double y0 = sw_strength(bi - 1, nwin, wins, lo, dt, dts), y2 = sw_strength(bi + 1, nwin, wins, lo, dt, dts);
  const double x0 = ntc[3 * (size_t)bi], x1 = ntc[3 * (size_t)bi + 1], x2 = ntc[3 * (size_t)bi + 2];
  const double d01 = (bv - y0) / (x1 - x0), d12 = (y2 - bv) / (x2 - x1);
  const double c2 = (d12 - d01) / (x2 - x0);
  const double c1 = d01 - c2 * (x0 + x1);
  const double c0 = y0 - x0 * (d01 - c2 * x1);
  int cnt = nf[bi];
  cnt = cnt < 1 ? 1 : (cnt > nfmax ? nfmax : cnt);
  double fv = -INFINITY;
  int fi = 0x7fffffff;
  if (lane < cnt) {
    const double xf = nftc[(size_t)bi * nfmax + lane];
    fv = (c2 * xf + c1) * xf + c0;   // Horner, as numpy.polyval
    fi = lane;
  }
  wave_first_max(fv, fi);
  if (live && lane == 0) {
    p[it] = ptab[(size_t)bi * nfmax + fi];
    s[it] = fv;
  }
}
}  // namespace eaqhm

using namespace eaqhm;

static int sw_log2(int w) {
  int l = 0;
  while ((1 << l) < w) ++l;
  return l;
}

extern "C" int eaqhm_swipe_loudness(eaqhm_ctx* ctx, const double* x, int64_t n, int32_t w, int32_t hop, int64_t pad,
                                    int64_t nframes, const double* window, double fs, double sumw2, const int32_t* lo,
                                    const double* xlo, const double* df, int32_t nE, double* L, int64_t ld) {
  if (!ctx) return EAQHM_EINVAL;
  if (!x || !window || !lo || !xlo || !df || !L) return ctx->fail(EAQHM_EINVAL, "eaqhm_swipe_loudness: bad argument");
  const int64_t lim = ((int64_t)1 << 31) - 1;
  if (n < 1 || w < 8 || w > EAQHM_SWIPE_WMAX || (w & (w - 1)) || hop < 1 || hop > w || pad < 0 || pad > lim ||
      nframes < 1 || nframes > lim || nE < 1 || nE > EAQHM_SWIPE_EMAX || ld < nE || !(fs > 0.0) || !(sumw2 > 0.0))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_swipe_loudness: need n >= 1, w a power of two in [8, 8192], 1 <= hop <= w, "
                                   "0 <= pad < 2^31, 1 <= nframes < 2^31, 1 <= nE <= 1024, ld >= nE, fs > 0, sumw2 > 0");
  const int logw = sw_log2(w);
  if (w <= 256) {
    const size_t lds = (size_t)4 * sw_region(w, nE, 64) * sizeof(double);
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_swipe_loudness_kernel<64>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(eaqhm_swipe_loudness_kernel<64>, dim3((unsigned)((nframes + 3) / 4)), dim3(256), lds, ctx->stream,
                       x, (i64)n, (int)w, logw, (int)hop, (i64)pad, (i64)nframes, window, fs, sumw2, (const int*)lo, xlo,
                       df, (int)nE, L, (i64)ld);
  } else {
    const size_t lds = (size_t)sw_region(w, nE, 256) * sizeof(double);
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_swipe_loudness_kernel<256>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(eaqhm_swipe_loudness_kernel<256>, dim3((unsigned)nframes), dim3(256), lds, ctx->stream, x, (i64)n,
                       (int)w, logw, (int)hop, (i64)pad, (i64)nframes, window, fs, sumw2, (const int*)lo, xlo, df, (int)nE,
                       L, (i64)ld);
  }
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_swipe_scores(eaqhm_ctx* ctx, const double* K, int32_t cand, int64_t ldk, const double* L,
                                  int64_t nframes, int64_t ldl, int32_t nE, double* Si) {
  if (!ctx) return EAQHM_EINVAL;
  if (!K || !L || !Si) return ctx->fail(EAQHM_EINVAL, "eaqhm_swipe_scores: bad argument");
  if (cand < 1 || cand > 4096 || nE < 1 || nE > 65536 || nframes < 1 || nframes > ((int64_t)1 << 31) - 1 || ldk < nE ||
      ldl < nE)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_swipe_scores: need 1 <= cand <= 4096, 1 <= nE <= 65536, 1 <= nframes < 2^31, "
                                   "ldk >= nE, ldl >= nE");
  hipLaunchKernelGGL(eaqhm_swipe_scores_kernel,
                     dim3((unsigned)((nframes + SW_TILE - 1) / SW_TILE), (unsigned)((cand + SW_TILE - 1) / SW_TILE)),
                     dim3(256), 0, ctx->stream, K, (int)cand, (i64)ldk, L, (i64)nframes, (i64)ldl, (int)nE, Si);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_swipe_pick(eaqhm_ctx* ctx, int32_t nwin, const double* const* Si, const int32_t* j0,
                                const int32_t* ncand, const int64_t* nframes, const double* const* mu,
                                const double* const* tshift, const double* t, int64_t T, int32_t npc, double pc0,
                                const double* ntc, const double* nftc, const double* ptab, const int32_t* nf,
                                int32_t nfmax, double* p, double* s, double* S) {
  if (!ctx) return EAQHM_EINVAL;
  if (!Si || !j0 || !ncand || !nframes || !mu || !tshift || !t || !ntc || !nftc || !ptab || !nf || !p || !s)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_swipe_pick: bad argument");
  const int64_t lim = ((int64_t)1 << 31) - 1;
  bool ok = nwin >= 1 && nwin <= EAQHM_SWIPE_WINDOWS && T >= 1 && T <= lim && npc >= 3 && npc <= 65536 && nfmax >= 1 &&
            nfmax <= EAQHM_SWIPE_FINE;
  SwipeWins a;
  memset(&a, 0, sizeof(a));
  for (int v = 0; ok && v < nwin; ++v) {
    ok = Si[v] && mu[v] && tshift[v] && nframes[v] >= 2 && nframes[v] <= lim && ncand[v] >= 1 && j0[v] >= 0 &&
         (int64_t)j0[v] + ncand[v] <= npc;
    a.win[v] = SwipeWin{Si[v], mu[v], tshift[v], (i64)nframes[v], (int)j0[v], (int)ncand[v]};
  }
  if (!ok)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_swipe_pick: need 1 <= nwin <= 8, 1 <= T < 2^31, 3 <= npc <= 65536, "
                                   "1 <= nfmax <= 64, and per window non-null arrays, nframes >= 2, candidates in [0, npc)");
  hipLaunchKernelGGL(eaqhm_swipe_pick_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, ctx->stream, a, (int)nwin, t,
                     (i64)T, (int)npc, pc0, ntc, nftc, ptab, (const int*)nf, (int)nfmax, p, s, S);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
