// eaqhm_onset.hip — the transient onset detector's three stages on the device.  gfx950 (MI355X) only.
//
//   eaqhm_onset_bands_kernel<G>  a group of G threads owns one frame: window, in-place complex FFT in LDS (imaginary part
//                                zero; eaqhm_swipe_loudness_kernel's transform, padded indexing and sincospi twiddles),
//                                P_k = |X_k|^2 inv_sumw2 in natural bin order into LDS, then thread b sums band b with k
//                                ascending and takes the logarithm.  G = 256 (a block) for w > 256, G = 64 (a wave, four
//                                frames a block) below.  A group reads and writes its own LDS region only, so a frame's
//                                row does not depend on its neighbours.
//   eaqhm_onset_flux_kernel      one thread per frame: the half-wave rectified difference to the frame `lag` earlier,
//                                summed over the bands in ascending order.
//   eaqhm_onset_peaks_kernel     one thread per frame: the first maximum of its window, the mean of its window in
//                                ascending frame order, the threshold.
//
// The host's NumPy model rounds every operation once, so nothing here may be contracted into an fma: flux and peaks are
// compared with the model bit for bit.  No atomics: every output word has one writer.
#include "eaqhm_common.h"
#include "../../include/eaqhm_onset.h"

#pragma clang fp contract(off)

namespace eaqhm {

typedef long long i64;

// LDS index of FFT element i: one double of padding after every 32, so that the late stages (four operands a butterfly
// 1, 2, 4 .. apart) spread over the banks.
__device__ inline int on_at(int i) { return i + (i >> 5); }
__host__ __device__ inline int on_padded(int w) { return w + (w >> 5); }
// doubles of one group's LDS region: re, im, P_0 .. P_{w/2}
__host__ __device__ inline int on_region(int w) { return 2 * on_padded(w) + (w >> 1) + 1; }

struct OnsetEdges {
  int k[EAQHM_ONSET_BANDS + 1];
};

template <int G>
__global__ void __launch_bounds__(256)
    eaqhm_onset_bands_kernel(const double* __restrict__ x, i64 n, int w, int logw, int hop, i64 nframes,
                             const double* __restrict__ window, double inv_sumw2, OnsetEdges edges, int B, double floor,
                             double* __restrict__ L, i64 ld) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int kb[EAQHM_ONSET_BANDS + 1];
  constexpr int FPB = 256 / G;   // frames of a block
  const int g = threadIdx.x / G, gt = threadIdx.x % G;
  const int wp = on_padded(w);
  double* re = lds + (size_t)g * on_region(w);
  double* im = re + wp;
  double* P = im + wp;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int b = 0; b <= EAQHM_ONSET_BANDS; ++b) kb[b] = edges.k[b];
  }
  const i64 m = (i64)blockIdx.x * FPB + g;
  const bool live = m < nframes;   // a group beyond the last frame transforms zeros and writes nothing
  const i64 start = m * hop - (w >> 1);
  for (int i = gt; i < w; i += G) {
    const i64 at = start + i;
    re[on_at(i)] = live && at >= 0 && at < n ? x[at] * window[i] : 0.0;
    im[on_at(i)] = 0.0;
  }
  __syncthreads();
  // decimation in frequency, in place: a radix-4 stage is two radix-2 stages fused, so the result is in bit-reversed order
  int S = w;
  for (; S >= 4; S >>= 2) {
    const int q = S >> 2;
    for (int b = gt; b < (w >> 2); b += G) {
      const int j = b & (q - 1), i0 = ((b - j) << 2) + j;
      const int p0 = on_at(i0), p1 = on_at(i0 + q), p2 = on_at(i0 + 2 * q), p3 = on_at(i0 + 3 * q);
      const double a0r = re[p0], a0i = im[p0], a1r = re[p1], a1i = im[p1];
      const double a2r = re[p2], a2i = im[p2], a3r = re[p3], a3i = im[p3];
      const double t0r = a0r + a2r, t0i = a0i + a2i, t1r = a1r + a3r, t1i = a1i + a3i;
      const double t2r = a0r - a2r, t2i = a0i - a2i, t3r = a1r - a3r, t3i = a1i - a3i;
      const double ur = t2r + t3i, ui = t2i - t3r;   // t2 - i t3
      const double vr = t2r - t3i, vi = t2i + t3r;   // t2 + i t3
      const double dr = t0r - t1r, di = t0i - t1i;
      // exp(-2 pi i m j / S), m = 1, 2, 3: the arguments j / (2 q) .. are exact
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
  if (S == 2) {
    for (int b = gt; b < (w >> 1); b += G) {
      const int p0 = on_at(2 * b), p1 = on_at(2 * b + 1);
      const double a0r = re[p0], a0i = im[p0], a1r = re[p1], a1i = im[p1];
      re[p0] = a0r + a1r;
      im[p0] = a0i + a1i;
      re[p1] = a0r - a1r;
      im[p1] = a0i - a1i;
    }
    __syncthreads();
  }
  for (int k = gt; k <= (w >> 1); k += G) {   // X_k sits at the bit-reversed position
    const int at = on_at((int)(__brev((unsigned)k) >> (32 - logw)));
    const double a = re[at], b = im[at];
    P[k] = (a * a + b * b) * inv_sumw2;
  }
  __syncthreads();
  if (live && gt < B) {   // B <= 64 <= G: one thread a band, k ascending
    double E = 0.0;
    for (int k = kb[gt]; k < kb[gt + 1]; ++k) E = E + P[k];
    L[(size_t)m * ld + gt] = log(E + floor);
  }
}

extern "C" __global__ void __launch_bounds__(256)
    eaqhm_onset_flux_kernel(const double* __restrict__ L, i64 nframes, i64 ld, int B, int lag, i64 whole_lo, i64 whole_hi,
                            double* __restrict__ d) {
  const i64 m = (i64)blockIdx.x * 256 + threadIdx.x;
  if (m >= nframes) return;
  double v = 0.0;
  if (m >= lag && m - lag >= whole_lo && m <= whole_hi) {
    const double* a = L + (size_t)m * ld;
    const double* p = L + (size_t)(m - lag) * ld;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
      const double t = a[b] - p[b];
      acc = acc + (t > 0.0 ? t : 0.0);
    }
    v = acc / (double)B;
  }
  d[m] = v;
}

extern "C" __global__ void __launch_bounds__(256)
    eaqhm_onset_peaks_kernel(const double* __restrict__ d, i64 nframes, int pre_max, int post_max, int pre_avg,
                             int post_avg, double delta, unsigned char* __restrict__ flag) {
  const i64 m = (i64)blockIdx.x * 256 + threadIdx.x;
  if (m >= nframes) return;
  const double v = d[m];
  const i64 last = nframes - 1;
  bool ok = v > 0.0;
  const i64 m0 = m - pre_max < 0 ? 0 : m - pre_max, m1 = m + post_max > last ? last : m + post_max;
  for (i64 j = m0; ok && j < m; ++j) ok = !(d[j] >= v);   // ties go to the first
  for (i64 j = m + 1; ok && j <= m1; ++j) ok = !(d[j] > v);
  if (ok) {
    const i64 a0 = m - pre_avg < 0 ? 0 : m - pre_avg, a1 = m + post_avg > last ? last : m + post_avg;
    double acc = 0.0;
    for (i64 j = a0; j <= a1; ++j) acc = acc + d[j];
    const double mean = acc / (double)(a1 - a0 + 1);
    ok = v >= mean + delta;
  }
  flag[m] = ok ? 1 : 0;
}
}  // namespace eaqhm

using namespace eaqhm;

extern "C" int eaqhm_onset_bands(eaqhm_ctx* ctx, const double* x, int64_t n, int32_t w, int32_t hop, int64_t nframes,
                                 const double* window, double inv_sumw2, const int32_t* k, int32_t B, double floor,
                                 double* L, int64_t ld) {
  if (!ctx) return EAQHM_EINVAL;
  if (!x || !window || !k || !L) return ctx->fail(EAQHM_EINVAL, "eaqhm_onset_bands: bad argument");
  const int64_t lim = ((int64_t)1 << 31) - 1;
  bool ok = n >= 1 && w >= EAQHM_ONSET_WMIN && w <= EAQHM_ONSET_WMAX && !(w & (w - 1)) && hop >= 1 &&
            hop <= EAQHM_ONSET_HOP && nframes >= 1 && nframes <= lim && B >= 1 && B <= EAQHM_ONSET_BANDS && ld >= B &&
            inv_sumw2 > 0.0 && inv_sumw2 <= 1.79769313486231570815e308 && floor > 0.0 && floor <= 1.79769313486231570815e308;
  OnsetEdges e;
  memset(&e, 0, sizeof(e));
  if (ok) ok = k[0] >= 0 && k[B] <= (w >> 1) + 1;
  for (int b = 0; ok && b < B; ++b) ok = k[b] < k[b + 1];
  if (!ok)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_onset_bands: need n >= 1, w a power of two in [32, 2048], 1 <= hop <= 4096, "
                                   "1 <= nframes < 2^31, 1 <= B <= 64, ld >= B, inv_sumw2 > 0, floor > 0, and edges "
                                   "0 <= k[0] < k[1] < .. < k[B] <= w/2 + 1");
  for (int b = 0; b <= B; ++b) e.k[b] = k[b];
  int logw = 0;
  while ((1 << logw) < w) ++logw;
  if (w <= 256) {
    const size_t lds = (size_t)4 * on_region(w) * sizeof(double);
    hipLaunchKernelGGL(eaqhm_onset_bands_kernel<64>, dim3((unsigned)((nframes + 3) / 4)), dim3(256), lds, ctx->stream, x,
                       (i64)n, (int)w, logw, (int)hop, (i64)nframes, window, inv_sumw2, e, (int)B, floor, L, (i64)ld);
  } else {
    const size_t lds = (size_t)on_region(w) * sizeof(double);   // 41.0 KB at w = 2048: under the 64 KB a launch gets unasked
    hipLaunchKernelGGL(eaqhm_onset_bands_kernel<256>, dim3((unsigned)nframes), dim3(256), lds, ctx->stream, x, (i64)n,
                       (int)w, logw, (int)hop, (i64)nframes, window, inv_sumw2, e, (int)B, floor, L, (i64)ld);
  }
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_onset_flux(eaqhm_ctx* ctx, const double* L, int64_t nframes, int64_t ld, int32_t B, int32_t lag,
                                int64_t whole_lo, int64_t whole_hi, double* d) {
  if (!ctx) return EAQHM_EINVAL;
  if (!L || !d) return ctx->fail(EAQHM_EINVAL, "eaqhm_onset_flux: bad argument");
  if (nframes < 1 || nframes > ((int64_t)1 << 31) - 1 || B < 1 || B > EAQHM_ONSET_BANDS || ld < B || lag < 1 ||
      lag > EAQHM_ONSET_LAG)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_onset_flux: need 1 <= nframes < 2^31, 1 <= B <= 64, ld >= B, 1 <= lag <= 16");
  hipLaunchKernelGGL(eaqhm_onset_flux_kernel, dim3((unsigned)((nframes + 255) / 256)), dim3(256), 0, ctx->stream, L,
                     (i64)nframes, (i64)ld, (int)B, (int)lag, (i64)whole_lo, (i64)whole_hi, d);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_onset_peaks(eaqhm_ctx* ctx, const double* d, int64_t nframes, int32_t pre_max, int32_t post_max,
                                 int32_t pre_avg, int32_t post_avg, double delta, uint8_t* flag) {
  if (!ctx) return EAQHM_EINVAL;
  if (!d || !flag) return ctx->fail(EAQHM_EINVAL, "eaqhm_onset_peaks: bad argument");
  const int S = EAQHM_ONSET_SPAN;
  if (nframes < 1 || nframes > ((int64_t)1 << 31) - 1 || pre_max < 0 || pre_max > S || post_max < 0 || post_max > S ||
      pre_avg < 0 || pre_avg > S || post_avg < 0 || post_avg > S || !(delta >= 0.0) || delta > 1.79769313486231570815e308)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_onset_peaks: need 1 <= nframes < 2^31, pre_max, post_max, pre_avg, post_avg in "
                                   "[0, 64], delta finite and >= 0");
  hipLaunchKernelGGL(eaqhm_onset_peaks_kernel, dim3((unsigned)((nframes + 255) / 256)), dim3(256), 0, ctx->stream, d,
                     (i64)nframes, (int)pre_max, (int)post_max, (int)pre_avg, (int)post_avg, delta, flag);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
