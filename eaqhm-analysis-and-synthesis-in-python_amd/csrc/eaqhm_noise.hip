// eaqhm_noise.hip — the stochastic component: an all-pole (LPC) envelope and a gain per short frame of
// the residual s - s_recon, and its resynthesis as filtered white noise under a time map.  Not in the reference.
//   eaqhm_noise_analyse_kernel   one wave per frame: windowed frame in LDS, lane l owns lag l, Levinson-Durbin in the wave
//   eaqhm_noise_filter_kernel    one lane per output frame: the all-pole lattice, state and coefficients in LDS
//   eaqhm_noise_combine_kernel   one thread per output sample: cross-fade of the two frames that cover it
//   eaqhm_noise_warp_kernel      one wave per frame: the frame's spectrum warped by alpha on a grid in LDS, lane l owns
//                                lag l of its autocorrelation, Levinson-Durbin in the wave
//   eaqhm_noise_envelope_kernel  one wave per frame, lanes over the frequency grid: the warped log power spectrum
//   eaqhm_noise_warp_map_kernel, eaqhm_noise_envelope_map_kernel  the same two bodies with the piecewise-linear map of
//                                DESIGN.md §10.3 (eaqhm_warp.h) as the read frequency in place of w / alpha
//   eaqhm_noise_cepstrum_kernel  one wave per frame: the cepstrum of the frame's log spectrum by the LPC-to-cepstrum
//                                recursion, lanes over the terms of each step
//   eaqhm_noise_from_cepstrum_kernel<WARP>  one wave per row: the spectrum of a cepstral row on the warp kernel's grid
//                                by Clenshaw's recurrence, then that kernel's lag sums and Levinson-Durbin recursion;
//                                WARP: the row lies on the all-pass warped axis (§9.8)
//   eaqhm_noise_modulation_kernel   one wave per frame, lanes over the frame's samples: the Fourier coefficients of the
//                                   residual's power over the fundamental's phase
//   eaqhm_noise_combine_mod_kernel  the combine kernel with each frame's pitch-synchronous gain g_q(n')
#include "eaqhm_common.h"
#include "eaqhm_warp.h"
#include "eaqhm_wave.h"

// The synthesis follows the NumPy model of the definition operation by operation (no fused multiply-add), so the two
// differ only where a library function does (cos); the autocorrelation sums ask for their FMAs by name.
#pragma clang fp contract(off)

namespace eaqhm {

constexpr int NA_WAVES = 4;   // frames (waves) per block of the analysis kernel
constexpr int NA_PAD = 64;    // zeros in front of each wave's frame: x[v - l] for v < l reads them (l <= 63)

// LDS: NA_WAVES x (NA_PAD + 4 hop) doubles
extern "C" __global__ void __launch_bounds__(64 * NA_WAVES)
    eaqhm_noise_analyse_kernel(const double* __restrict__ e, long long L, int H, int p, int Nf,
                               double* __restrict__ sigma, double* __restrict__ refl) {
  extern __shared__ double na_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int W = 4 * H;
  double* x = na_lds + (size_t)wave * (NA_PAD + W);
  const int m = blockIdx.x * NA_WAVES + wave;
  const bool live = m < Nf;
  const long long base = (long long)m * H - 2 * H;
  x[lane] = 0.0;
  double sw2 = 0.0;
  for (int v = lane; v < W; v += 64) {
    const double w = 0.5 - 0.5 * cospi((double)(2 * v + 1) / (double)W);
    const long long t = base + v;
    const double ev = (live && t >= 0 && t < L) ? e[t] : 0.0;
    x[NA_PAD + v] = w * ev;
    sw2 += w * w;
  }
  __syncthreads();
  if (!live) return;

  // r[l] on lane l: x[v] is one address for the wave, x[v - l] consecutive addresses across lanes
  const double* xv = x + NA_PAD;
  const double* xl = x + NA_PAD - lane;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  for (int v = 0; v < W; v += 4) {
    r0 = fma(xv[v], xl[v], r0);
    r1 = fma(xv[v + 1], xl[v + 1], r1);
    r2 = fma(xv[v + 2], xl[v + 2], r2);
    r3 = fma(xv[v + 3], xl[v + 3], r3);
  }
  double r = (r0 + r1) + (r2 + r3);
  sw2 = wave_sum(sw2);

  // Levinson-Durbin in the wave (eaqhm_wave.h), r[0] inflated by the -90 dB white floor
  const double r00 = __shfl(r, 0, 64);
  double kk = 0.0, E = 0.0;
  if (r00 > 0.0) E = levinson_lanes<true>(r, p, lane, kk);
  if (lane == 0) sigma[m] = r00 > 0.0 ? sqrt(E / sw2) : 0.0;
  if (lane >= 1 && lane <= p) refl[(size_t)m * p + (lane - 1)] = kk;
}

// the white excitation: a pure function of (seed, n), exact in integers (splitmix64), uniform with unit variance
__device__ __forceinline__ double white(unsigned long long seed, long long n) {
  unsigned long long z = seed + ((unsigned long long)n + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return ((double)(z >> 11) * 0x1p-53 - 0.5) * 3.4641016151377544;
}

// Output frames [q_lo, q_lo + nq): lane = frame.  LDS [stage][lane]: k_1..k_p, then b_0..b_{p-1} (b_p is never read).
// Y[u][frame], u = 0..2H-1: the 2H samples the frame keeps, n' = qH - H + u.
extern "C" __global__ void __launch_bounds__(64)
    eaqhm_noise_filter_kernel(const double* __restrict__ sigma, const double* __restrict__ refl, int Nf, int H, int p,
                              const double* __restrict__ tau, unsigned long long seed, int q_lo, int nq,
                              double* __restrict__ Y) {
  extern __shared__ double ns_lds[];
  const int lane = threadIdx.x;
  const int qi = blockIdx.x * 64 + lane;
  if (qi >= nq) return;
  double* kq = ns_lds + lane;
  double* b = ns_lds + (size_t)p * 64 + lane;
  const long long q = (long long)q_lo + qi;
  const double mu = tau[q] / (double)H;
  long long m0 = (long long)floor(mu);
  m0 = m0 < 0 ? 0 : (m0 > Nf - 1 ? Nf - 1 : m0);        // tau is the caller's: never index outside the model
  const long long m1 = m0 + 1 > Nf - 1 ? Nf - 1 : m0 + 1;
  const double fr = fmin(mu - (double)m0, 1.0);
  const double w0 = 1.0 - fr;
  const double sg = w0 * sigma[m0] + fr * sigma[m1];
  for (int i = 0; i < p; ++i) {
    kq[i * 64] = w0 * refl[m0 * p + i] + fr * refl[m1 * p + i];
    b[i * 64] = 0.0;
  }
  const long long n0 = q * H - 3 * H;
  for (int t = 0; t < 4 * H; ++t) {
    const long long n = n0 + t;
    double f = n >= 0 ? sg * white(seed, n) : 0.0;
    f = f - kq[(p - 1) * 64] * b[(p - 1) * 64];
#pragma unroll 4
    for (int i = p - 1; i >= 1; --i) {
      const double k = kq[(i - 1) * 64], bp = b[(i - 1) * 64];
      f = f - k * bp;
      b[i * 64] = bp + k * f;
    }
    b[0] = f;
    if (t >= 2 * H) Y[(size_t)(t - 2 * H) * nq + qi] = f;
  }
}

__device__ __forceinline__ double fade(int u, int H) { return 0.5 - 0.5 * cos(2.0 * M_PI * (double)u / (double)(2 * H)); }

extern "C" __global__ void __launch_bounds__(256)
    eaqhm_noise_combine_kernel(const double* __restrict__ Y, int H, int q_lo, int nq, int Nq, long long t_lo,
                               long long t_hi, double* __restrict__ out, int accumulate) {
  const long long n = t_lo + (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= t_hi) return;
  const long long q = n / H;
  const int j = (int)(n - q * H);
  const int qi = (int)(q - q_lo);
  double val = fade(H + j, H) * Y[(size_t)(H + j) * nq + qi];
  if (q + 1 < Nq) val = val + fade(j, H) * Y[(size_t)j * nq + qi + 1];
  out[n] = accumulate ? out[n] + val : val;
}

// ---- the formant warp of the model (tests/noise_warp_ref.py)
constexpr int NW_M = 1024;    // grid intervals on [0, pi] (M of the definition)
constexpr int NW_WAVES = 8;   // frames (waves) per block of the warp kernel
constexpr int NE_WAVES = 4;   // frames (waves) per block of the envelope kernel

// |A(e^{jw})|^2, a[0..p] in LDS (one address for the wave).  One sincos, then e^{jiw} by rotation: its error grows like
// i ulp, the size of the rounding of the product i w in the model.
__device__ __forceinline__ double poly_power(const double* a, int p, double w) {
  double s, c;
  sincos(w, &s, &c);
  double re = 1.0, im = 0.0, ci = c, si = s;
  for (int i = 1; i <= p; ++i) {
    const double ai = a[i];
    re = fma(ai, ci, re);
    im = fma(ai, si, im);
    const double cn = fma(ci, c, -(si * s));
    si = fma(si, c, ci * s);
    ci = cn;
  }
  return re * re + im * im;
}

// Where a frame's spectrum is read: `grid(t)` is the angle for grid point t of the warp, `angle(f)` the one for the
// normalised frequency f of the envelope readout, `unit()` says that the frame passes through bit for bit; `load`
// fetches what the frame needs from memory where the body asks for it.
struct ScaleRead {   // §10.1: the frequency axis divided by alpha
  const double* __restrict__ alpha;
  double al;
  __device__ __forceinline__ void load(bool live, int m) { al = live ? alpha[m] : 1.0; }
  __device__ __forceinline__ bool unit() const { return al == 1.0; }
  __device__ __forceinline__ double grid(int t) const { return fmin(M_PI * (double)t / (double)NW_M / al, M_PI); }
  __device__ __forceinline__ double angle(double f) const { return (2.0 * M_PI) * fmin(f / al, 0.5); }
};

struct MapRead {     // §10.3: the inverse of the piecewise-linear map, breakpoints in cycles per sample
  WarpRow W;
  __device__ __forceinline__ void load(bool, int) {}   // the kernel staged the row in LDS
  __device__ __forceinline__ bool unit() const { return W.ident; }
  __device__ __forceinline__ double grid(int t) const {
    return fmin((2.0 * M_PI) * warp_inverse(W, (double)t / (double)(2 * NW_M)), M_PI);
  }
  __device__ __forceinline__ double angle(double f) const { return fmin((2.0 * M_PI) * warp_inverse(W, f), M_PI); }
};

// The warp of one frame by one wave (the body of both warp kernels).  tab: the cosine table cos(pi j / M), j = 0..M,
// shared by the block; P: the wave's P'[0..M]; a: the wave's a[0..63].  Every wave of the block reaches both barriers.
template <class Read>
__device__ __forceinline__ void noise_warp_frame(const double* __restrict__ sigma, const double* __restrict__ refl,
                                                 int p, int lane, int m, bool live, Read rd, double* tab, double* P,
                                                 double* a, double* __restrict__ sigma_out,
                                                 double* __restrict__ refl_out) {
  for (int j = threadIdx.x; j <= NW_M; j += 64 * NW_WAVES) tab[j] = cospi((double)j / (double)NW_M);
  const double sg = live ? sigma[m] : 0.0;
  rd.load(live, m);
  const double kin = (live && lane >= 1 && lane <= p) ? refl[(size_t)m * p + (lane - 1)] : 0.0;
  const bool unit = rd.unit();
  const bool work = live && !unit && sg > 0.0;     // uniform over the wave
  if (work) a[lane] = stepup_lanes(kin, p, lane);
  __syncthreads();
  if (work) {
    for (int t = lane; t <= NW_M; t += 64) {
      const double w = rd.grid(t);
      P[t] = sg * sg / poly_power(a, p, w);
    }
  }
  __syncthreads();
  if (!live) return;
  if (!work) {   // a unit read: the frame bit for bit; otherwise a silent frame
    if (lane == 0) sigma_out[m] = unit ? sg : 0.0;
    if (lane >= 1 && lane <= p) refl_out[(size_t)m * p + (lane - 1)] = unit ? kin : 0.0;
    return;
  }

  // r'[l] on lane l: P'[t] is one address for the wave; the table index (l t) mod 2M folds onto [0, M].  Where the read
  // angle is held at pi over part of the grid (alpha < 1, a map that passes fs/2) the terms of lag 0 are one constant
  // there, and a running sum that adds one constant 128 times rounds the same way every time: up to 150 x the model's
  // own rounding error.  Such a frame sets its running sums aside every 64 grid points (16 terms each);
  // a frame without a held stretch is summed in one run, bit for bit as it always was.
  auto ct = [&](int t) {
    const int idx = (lane * t) & (2 * NW_M - 1);
    return tab[idx > NW_M ? 2 * NW_M - idx : idx];
  };
  const bool held = rd.grid(NW_M - 1) == M_PI;     // uniform over the wave
  double r0 = 0.5 * P[0], r1 = 0.0, r2 = 0.0, r3 = ((lane & 1) ? -0.5 : 0.5) * P[NW_M];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int t = 1; t + 3 < NW_M; t += 4) {
    r0 = fma(P[t], ct(t), r0);
    r1 = fma(P[t + 1], ct(t + 1), r1);
    r2 = fma(P[t + 2], ct(t + 2), r2);
    r3 = fma(P[t + 3], ct(t + 3), r3);
    if (held && (t & 63) == 61) {
      s0 += r0;
      s1 += r1;
      s2 += r2;
      s3 += r3;
      r0 = r1 = r2 = r3 = 0.0;
    }
  }
  r0 = fma(P[NW_M - 3], ct(NW_M - 3), r0);
  r1 = fma(P[NW_M - 2], ct(NW_M - 2), r1);
  r2 = fma(P[NW_M - 1], ct(NW_M - 1), r2);
  if (held) {
    r0 += s0;
    r1 += s1;
    r2 += s2;
    r3 += s3;
  }
  const double r = ((r0 + r1) + (r2 + r3)) / (double)NW_M;

  double kk = 0.0;
  const double E = levinson_lanes(r, p, lane, kk);
  if (lane == 0) sigma_out[m] = sqrt(E);
  if (lane >= 1 && lane <= p) refl_out[(size_t)m * p + (lane - 1)] = kk;
}

// LDS (static): the cosine table (shared by the block), and per wave P'[0..M] and a[0..63]
extern "C" __global__ void __launch_bounds__(64 * NW_WAVES)
    eaqhm_noise_warp_kernel(const double* __restrict__ sigma, const double* __restrict__ refl, int Nf, int p,
                            const double* __restrict__ alpha, double* __restrict__ sigma_out,
                            double* __restrict__ refl_out) {
  __shared__ double tab[NW_M + 1];
  __shared__ double Pw[NW_WAVES][NW_M + 2];
  __shared__ double aw[NW_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * NW_WAVES + wave;
  const bool live = m < Nf;
  const ScaleRead rd{alpha, 1.0};
  noise_warp_frame(sigma, refl, p, lane, m, live, rd, tab, Pw[wave], aw[wave], sigma_out, refl_out);
}

// the same with frame m's row of the map; LDS: 2 x WARP_BMAX doubles more per wave and WARP_BMAX for the block
extern "C" __global__ void __launch_bounds__(64 * NW_WAVES)
    eaqhm_noise_warp_map_kernel(const double* __restrict__ sigma, const double* __restrict__ refl, int Nf, int p,
                                const double* __restrict__ f_in, const double* __restrict__ f_out, int B,
                                double* __restrict__ sigma_out, double* __restrict__ refl_out) {
  __shared__ double tab[NW_M + 1];
  __shared__ double Pw[NW_WAVES][NW_M + 2];
  __shared__ double aw[NW_WAVES][64];
  __shared__ double wy[NW_WAVES][WARP_BMAX], ws[NW_WAVES][WARP_BMAX], wx[WARP_BMAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * NW_WAVES + wave;
  const bool live = m < Nf;
  warp_stage_x(f_in, B, threadIdx.x, wx);
  const bool ident = live ? warp_stage(f_in, f_out + (size_t)m * B, B, lane, wy[wave], ws[wave]) : true;
  const MapRead rd{WarpRow{wx, wy[wave], ws[wave], B, ident}};   // read after the body's first barrier
  noise_warp_frame(sigma, refl, p, lane, m, live, rd, tab, Pw[wave], aw[wave], sigma_out, refl_out);
}

// The envelope readout of one frame by one wave (the body of both envelope kernels): out[m][t] = 2 ln sigma_m -
// ln |A_m(e^{jw})|^2 at w = rd.angle(fnorm[t]); -inf rows for silent frames.  a: the wave's a[0..63].
template <class Read>
__device__ __forceinline__ void noise_envelope_frame(const double* __restrict__ sigma, const double* __restrict__ refl,
                                                     int p, int lane, int m, bool live, Read rd, double* a,
                                                     const double* __restrict__ fnorm, int F,
                                                     double* __restrict__ out) {
  const double kin = (live && lane >= 1 && lane <= p) ? refl[(size_t)m * p + (lane - 1)] : 0.0;
  a[lane] = stepup_lanes(kin, p, lane);
  __syncthreads();
  if (!live) return;
  const double sg = sigma[m];
  rd.load(true, m);
  const double ls = 2.0 * log(sg);
  double* row = out + (size_t)m * F;
  for (int t = lane; t < F; t += 64) {
    const double w = rd.angle(fnorm[t]);
    row[t] = sg > 0.0 ? ls - log(poly_power(a, p, w)) : -INFINITY;
  }
}

// w = 2 pi min(fnorm[t] / alpha_m, 1/2)
extern "C" __global__ void __launch_bounds__(64 * NE_WAVES)
    eaqhm_noise_envelope_kernel(const double* __restrict__ sigma, const double* __restrict__ refl, int Nf, int p,
                                const double* __restrict__ alpha, const double* __restrict__ fnorm, int F,
                                double* __restrict__ out) {
  __shared__ double aw[NE_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * NE_WAVES + wave;
  const bool live = m < Nf;
  const ScaleRead rd{alpha, 1.0};
  noise_envelope_frame(sigma, refl, p, lane, m, live, rd, aw[wave], fnorm, F, out);
}

// w = min(2 pi V_m(fnorm[t]), pi)
extern "C" __global__ void __launch_bounds__(64 * NE_WAVES)
    eaqhm_noise_envelope_map_kernel(const double* __restrict__ sigma, const double* __restrict__ refl, int Nf, int p,
                                    const double* __restrict__ f_in, const double* __restrict__ f_out, int B,
                                    const double* __restrict__ fnorm, int F, double* __restrict__ out) {
  __shared__ double aw[NE_WAVES][64];
  __shared__ double wy[NE_WAVES][WARP_BMAX], ws[NE_WAVES][WARP_BMAX], wx[WARP_BMAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * NE_WAVES + wave;
  const bool live = m < Nf;
  warp_stage_x(f_in, B, threadIdx.x, wx);
  const bool ident = live ? warp_stage(f_in, f_out + (size_t)m * B, B, lane, wy[wave], ws[wave]) : true;
  const MapRead rd{WarpRow{wx, wy[wave], ws[wave], B, ident}};   // read after the body's barrier
  noise_envelope_frame(sigma, refl, p, lane, m, live, rd, aw[wave], fnorm, F, out);
}

// ---- the noise model to and from cepstral rows (tests/noise_cepstrum_ref.py)
constexpr int NC_WAVES = 4;   // frames (waves) per block of the cepstrum kernel

// ceps[m][0..Q] of C_m(w) = ln(sigma_m / |A_m(e^{jw})|) = c_0 + 2 sum_q c_q cos(q w): c_0 = ln sigma_m, c_q = h_q / 2 with
// h_n = -a_n - (sum_{k=1}^{n-1} (k h_k) a_{n-k}) / n, a_j = 0 past p (the LPC-to-cepstrum recursion).  Lanes over k:
// lane k keeps k h_k in a register, step n reads a[n - lane] (consecutive LDS addresses) and the sum is wave_sum's
// butterfly, so a step costs one product and six cross-lane adds whatever p is.  A silent frame gives (-inf, 0, .., 0).
// LDS (static): a[0..63] per wave.  Every wave of the block reaches the barrier.
extern "C" __global__ void __launch_bounds__(64 * NC_WAVES)
    eaqhm_noise_cepstrum_kernel(const double* __restrict__ sigma, const double* __restrict__ refl, int Nf, int p, int Q,
                                double* __restrict__ ceps) {
  __shared__ double aw[NC_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * NC_WAVES + wave;
  const bool live = m < Nf;
  const double kin = (live && lane >= 1 && lane <= p) ? refl[(size_t)m * p + (lane - 1)] : 0.0;
  double* a = aw[wave];
  a[lane] = stepup_lanes(kin, p, lane);            // zero on the lanes past p
  __syncthreads();
  if (!live) return;
  const double sg = sigma[m];
  double kh = 0.0, cq = 0.0;                       // lane k: k h_k and c_k
  for (int n = 1; n <= Q; ++n) {
    const bool in = lane >= 1 && lane < n;
    const double ak = a[in ? n - lane : 0];
    const double s = wave_sum(in ? kh * ak : 0.0);
    const double h = -a[n] - s / (double)n;
    if (lane == n) {
      kh = (double)n * h;
      cq = 0.5 * h;
    }
  }
  if (lane == 0) cq = log(sg);
  if (!(sg > 0.0)) cq = lane == 0 ? -INFINITY : 0.0;
  if (lane <= Q) ceps[(size_t)m * (Q + 1) + lane] = cq;
}

// The way back, by the route of the warp kernel: P[t] = exp(2 (C(w_t) - c_0)) = exp(4 sum_q c_q cos(q w_t)) on the grid
// w_t = pi t / M (Clenshaw's recurrence from cos w_t, which is the block's table entry t), the lag sums and the
// Levinson-Durbin recursion of noise_warp_frame (without the inflation of r[0]; the lag sums are written a second time,
// without that body's held stretches), and sigma = exp(c_0) sqrt(E).  c_0 never enters P: the reflection coefficients
// do not depend on it.  An empty row (c_0 = -inf) gives a silent frame.  LDS (static): the cosine table (shared by the
// block), and per wave P[0..M] and the row c[0..63]: 77 968 bytes, two blocks per CU.  Every wave of the block reaches
// both barriers.
// WARP (include/eaqhm_cepwarp.h): the row lies on the all-pass warped axis with parameter cep_a (0.0 and
// not read without it), so Clenshaw runs from cos Omega_a(w_t) = (v - u)(v + u) / (u^2 + v^2), u = (1 + a) sin(w_t / 2),
// v = (1 - a) cos(w_t / 2), taken at the half angle itself (one sincospi per cell beside the Q steps of the recurrence:
// the table's cos w_t would lose the stretched band to cancellation at |a| near 0.9).  The lag sums and the recursion
// read the table either way.
template <bool WARP>
__global__ void __launch_bounds__(64 * NW_WAVES)
    eaqhm_noise_from_cepstrum_kernel(const double* __restrict__ ceps, int Nf, int Q, int p,
                                     double* __restrict__ sigma_out, double* __restrict__ refl_out, double cep_a) {
  __shared__ double tab[NW_M + 1];
  __shared__ double Pw[NW_WAVES][NW_M + 2];
  __shared__ double cw[NW_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * NW_WAVES + wave;
  const bool live = m < Nf;
  for (int j = threadIdx.x; j <= NW_M; j += 64 * NW_WAVES) tab[j] = cospi((double)j / (double)NW_M);
  const double cl = (live && lane <= Q) ? ceps[(size_t)m * (Q + 1) + lane] : 0.0;
  double* c = cw[wave];
  double* P = Pw[wave];
  c[lane] = cl;
  const double c0 = __shfl(cl, 0, 64);
  const bool work = live && c0 != -INFINITY;       // uniform over the wave
  __syncthreads();
  if (work) {
    for (int t = lane; t <= NW_M; t += 64) {
      double cw2;
      if constexpr (WARP) {
        double sh, ch;
        sincospi((double)t / (double)(2 * NW_M), &sh, &ch);
        const double u = (1.0 + cep_a) * sh, v = (1.0 - cep_a) * ch;
        cw2 = 2.0 * (((v - u) * (v + u)) / (u * u + v * v));
      } else {
        cw2 = 2.0 * tab[t];
      }
      double b1 = 0.0, b2 = 0.0;
      for (int q = Q; q >= 1; --q) {               // one LDS address for the wave: a broadcast
        const double b0 = c[q] + (cw2 * b1 - b2);
        b2 = b1;
        b1 = b0;
      }
      P[t] = exp(4.0 * (0.5 * cw2 * b1 - b2));
    }
  }
  __syncthreads();
  if (!live) return;
  if (!work) {
    if (lane == 0) sigma_out[m] = 0.0;
    if (lane >= 1 && lane <= p) refl_out[(size_t)m * p + (lane - 1)] = 0.0;
    return;
  }

  // r[l] on lane l, as in noise_warp_frame
  auto ct = [&](int t) {
    const int idx = (lane * t) & (2 * NW_M - 1);
    return tab[idx > NW_M ? 2 * NW_M - idx : idx];
  };
  double r0 = 0.5 * P[0], r1 = 0.0, r2 = 0.0, r3 = ((lane & 1) ? -0.5 : 0.5) * P[NW_M];
  for (int t = 1; t + 3 < NW_M; t += 4) {
    r0 = fma(P[t], ct(t), r0);
    r1 = fma(P[t + 1], ct(t + 1), r1);
    r2 = fma(P[t + 2], ct(t + 2), r2);
    r3 = fma(P[t + 3], ct(t + 3), r3);
  }
  r0 = fma(P[NW_M - 3], ct(NW_M - 3), r0);
  r1 = fma(P[NW_M - 2], ct(NW_M - 2), r1);
  r2 = fma(P[NW_M - 1], ct(NW_M - 1), r2);
  const double r = ((r0 + r1) + (r2 + r3)) / (double)NW_M;

  double kk = 0.0;
  const double E = levinson_lanes<false>(r, p, lane, kk);
  if (lane == 0) sigma_out[m] = exp(c0) * sqrt(E);
  if (lane >= 1 && lane <= p) refl_out[(size_t)m * p + (lane - 1)] = kk;
}

// ---- pitch-synchronous modulation of the noise (tests/noise_modulation_ref.py)
constexpr int NM_WAVES = 4;  // frames (waves) per block of the modulation kernel
constexpr int NM_MAX = 8;     // harmonics of the envelope (M of the definition) at most

// i of the definition: the instant nearest to input position x
__device__ __forceinline__ int nearest_instant(double x, double ti0, double D, int n) {
  const double r = rint((x - ti0) / D);
  return r < 0.0 ? 0 : (r > (double)(n - 1) ? n - 1 : (int)r);
}

// mod[m][2j], mod[m][2j+1] = Re, Im of c_{j+1} = sum_v u[v] exp(-2 pi i (j+1) Theta(mH - 2H + v)) / sum_v u[v],
// u = (w e)^2.  Order of the sums: lane l adds its samples v = l, l + 64, .. in increasing v, then the butterfly of
// wave_sum (partner lane ^ 32, 16, .. 1).  All NM_MAX harmonics are summed (registers, no indexing by M); M are stored.
extern "C" __global__ void __launch_bounds__(64 * NM_WAVES)
    eaqhm_noise_modulation_kernel(const double* __restrict__ e, long long L, int H, int Nf,
                                  const double* __restrict__ theta, const double* __restrict__ f0,
                                  const unsigned char* __restrict__ voiced, int n, double ti0, double D, double fs, int M,
                                  double* __restrict__ mod) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = blockIdx.x * NM_WAVES + wave;
  if (m >= Nf) return;
  double* row = mod + (size_t)m * 2 * M;
  const int W = 4 * H;
  const long long base = (long long)m * H - 2 * H;
  if (!voiced[nearest_instant((double)((long long)m * H), ti0, D, n)]) {   // uniform over the wave
    if (lane < 2 * M) row[lane] = 0.0;
    return;
  }
  double P = 0.0, re[NM_MAX], im[NM_MAX];
#pragma unroll
  for (int j = 0; j < NM_MAX; ++j) re[j] = im[j] = 0.0;
  for (int v = lane; v < W; v += 64) {
    const double w = 0.5 - 0.5 * cospi((double)(2 * v + 1) / (double)W);
    const long long t = base + v;
    const double x = w * ((t >= 0 && t < L) ? e[t] : 0.0);
    const double u = x * x;
    const double pos = (double)t;
    const int i = nearest_instant(pos, ti0, D, n);
    double th = theta[i] + f0[i] * (pos - (ti0 + (double)i * D)) / fs;
    th = th - floor(th);
    double s1, c1;
    sincos((2.0 * M_PI) * th, &s1, &c1);
    P = P + u;
    double cj = c1, sj = s1;
#pragma unroll
    for (int j = 0; j < NM_MAX; ++j) {
      re[j] = re[j] + u * cj;
      im[j] = im[j] - u * sj;
      const double cn = cj * c1 - sj * s1;
      sj = sj * c1 + cj * s1;
      cj = cn;
    }
  }
  P = wave_sum(P);
  const bool some = P > 0.0;
#pragma unroll
  for (int j = 0; j < NM_MAX; ++j) {
    const double cr = wave_sum(re[j]), ci = wave_sum(im[j]);
    if (j < M && lane == 2 * j) row[lane] = some ? cr / P : 0.0;
    if (j < M && lane == 2 * j + 1) row[lane] = some ? ci / P : 0.0;
  }
}

// g_q(n'), d = n' - qH: the coefficients blended between the model's frames as the filter kernel blends sigma and k;
// one sincos of the reduced phase, e^{2 pi i j phi} by rotation, as the model has it
__device__ __forceinline__ double mod_gain(const double* __restrict__ mod, int M, int Nf, int H, double tauq, double thq,
                                           double nuq, double d) {
  const double mu = tauq / (double)H;
  long long m0 = (long long)floor(mu);
  m0 = m0 < 0 ? 0 : (m0 > Nf - 1 ? Nf - 1 : m0);
  const long long m1 = m0 + 1 > Nf - 1 ? Nf - 1 : m0 + 1;
  const double fr = fmin(mu - (double)m0, 1.0);
  const double w0 = 1.0 - fr;
  const double* a = mod + (size_t)m0 * 2 * M;
  const double* b = mod + (size_t)m1 * 2 * M;
  double ph = thq + nuq * d;
  ph = ph - floor(ph);
  double s1, c1;
  sincos((2.0 * M_PI) * ph, &s1, &c1);
  double cj = c1, sj = s1, acc = 0.0;
  for (int j = 0; j < M; ++j) {
    const double cr = w0 * a[2 * j] + fr * b[2 * j];
    const double ci = w0 * a[2 * j + 1] + fr * b[2 * j + 1];
    acc = acc + (cr * cj - ci * sj);
    const double cn = cj * c1 - sj * s1;
    sj = sj * c1 + cj * s1;
    cj = cn;
  }
  return sqrt(fmax(0.01, 1.0 + 2.0 * acc));
}

extern "C" __global__ void __launch_bounds__(256)
    eaqhm_noise_combine_mod_kernel(const double* __restrict__ Y, int H, int q_lo, int nq, int Nq, long long t_lo,
                                   long long t_hi, double* __restrict__ out, int accumulate,
                                   const double* __restrict__ mod, int M, int Nf, const double* __restrict__ tau,
                                   const double* __restrict__ theta, const double* __restrict__ nu) {
  const long long n = t_lo + (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= t_hi) return;
  const long long q = n / H;
  const int j = (int)(n - q * H);
  const int qi = (int)(q - q_lo);
  double val = (fade(H + j, H) * mod_gain(mod, M, Nf, H, tau[q], theta[q], nu[q], (double)j)) * Y[(size_t)(H + j) * nq + qi];
  if (q + 1 < Nq)
    val = val + (fade(j, H) * mod_gain(mod, M, Nf, H, tau[q + 1], theta[q + 1], nu[q + 1], (double)(j - H))) *
                    Y[(size_t)j * nq + qi + 1];
  out[n] = accumulate ? out[n] + val : val;
}

}  // namespace eaqhm

using namespace eaqhm;

static bool noise_shape_ok(int32_t hop, int32_t order) {
  return hop >= 1 && hop <= 1024 && order >= 1 && order <= 63 && order < 4 * hop;
}

extern "C" int eaqhm_noise_analyse(eaqhm_ctx* ctx, const double* e, int64_t L, int32_t hop, int32_t order, double* sigma,
                                   double* refl) {
  if (!ctx) return EAQHM_EINVAL;
  if (!e || !sigma || !refl || L < 1) return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_analyse: bad argument");
  if (!noise_shape_ok(hop, order))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_analyse: need 1 <= hop <= 1024, 1 <= order <= 63, order < 4 hop");
  const int64_t Nf = (L - 1) / hop + 1;
  if (Nf > INT32_MAX - NA_WAVES) return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_analyse: too many frames");
  const size_t lds = (size_t)NA_WAVES * (NA_PAD + 4 * (size_t)hop) * sizeof(double);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_noise_analyse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  hipLaunchKernelGGL(eaqhm_noise_analyse_kernel, dim3((unsigned)((Nf + NA_WAVES - 1) / NA_WAVES)), dim3(64 * NA_WAVES), lds,
                     ctx->stream, e, (long long)L, (int)hop, (int)order, (int)Nf, sigma, refl);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

// mod, theta and nu given: the modulated cross-fade; none of them: the plain one, harmonics not read
extern "C" int eaqhm_noise_synth(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf, int32_t hop,
                                 int32_t order, const double* tau, int32_t Nq, uint64_t seed, int64_t L_out, int64_t t_lo,
                                 int64_t t_hi, double* out, int32_t accumulate, const double* mod, int32_t harmonics,
                                 const double* theta, const double* nu) {
  if (!ctx) return EAQHM_EINVAL;
  if (!sigma || !refl || !tau || !out || Nf < 1 || ((mod || theta || nu) && !(mod && theta && nu)))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_synth: bad argument");
  if (mod && (harmonics < 1 || harmonics > NM_MAX))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_synth: need 1 <= harmonics <= 8");
  if (!noise_shape_ok(hop, order))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_synth: need 1 <= hop <= 1024, 1 <= order <= 63, order < 4 hop");
  if (L_out <= 0 || (L_out - 1) / hop + 1 != (int64_t)Nq)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_synth: Nq must be (L_out - 1) / hop + 1");
  if (t_lo < 0 || t_hi > L_out || t_lo >= t_hi)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_synth: [t_lo, t_hi) outside [0, L_out)");
  // the frames that cover [t_lo, t_hi): sample n' lies in frames n' / hop and n' / hop + 1
  const int64_t q_lo = t_lo / hop;
  int64_t q_hi = (t_hi - 1) / hop + 1;
  if (q_hi > Nq - 1) q_hi = Nq - 1;
  const int nq = (int)(q_hi - q_lo + 1);
  if (int rc = ctx->reserve((size_t)nq * 2 * hop * sizeof(double))) return rc;
  double* Y = (double*)ctx->scratch;
  const size_t lds = (size_t)2 * order * 64 * sizeof(double);
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_noise_filter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  hipLaunchKernelGGL(eaqhm_noise_filter_kernel, dim3((unsigned)((nq + 63) / 64)), dim3(64), lds, ctx->stream, sigma, refl,
                     (int)Nf, (int)hop, (int)order, tau, (unsigned long long)seed, (int)q_lo, nq, Y);
  HIP_TRY(ctx, hipGetLastError());
  const dim3 grid((unsigned)((t_hi - t_lo + 255) / 256));
  if (mod)
    hipLaunchKernelGGL(eaqhm_noise_combine_mod_kernel, grid, dim3(256), 0, ctx->stream, (const double*)Y, (int)hop,
                       (int)q_lo, nq, (int)Nq, (long long)t_lo, (long long)t_hi, out, (int)(accumulate != 0), mod,
                       (int)harmonics, (int)Nf, tau, theta, nu);
  else
    hipLaunchKernelGGL(eaqhm_noise_combine_kernel, grid, dim3(256), 0, ctx->stream, (const double*)Y, (int)hop, (int)q_lo,
                       nq, (int)Nq, (long long)t_lo, (long long)t_hi, out, (int)(accumulate != 0));
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_noise_modulation(eaqhm_ctx* ctx, const double* e, int64_t L, int32_t hop, const double* theta,
                                      const double* f0, const uint8_t* voiced, int32_t No_ti, double ti0, double step,
                                      double fs, int32_t harmonics, double* mod) {
  if (!ctx) return EAQHM_EINVAL;
  if (!e || !theta || !f0 || !voiced || !mod || L < 1 || No_ti < 1)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_modulation: bad argument");
  if (hop < 1 || hop > 1024 || harmonics < 1 || harmonics > NM_MAX || !(step > 0.0) || !(fs > 0.0))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_modulation: need 1 <= hop <= 1024, 1 <= harmonics <= 8, step > 0, fs > 0");
  const int64_t Nf = (L - 1) / hop + 1;
  if (Nf > INT32_MAX - NM_WAVES) return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_modulation: too many frames");
  hipLaunchKernelGGL(eaqhm_noise_modulation_kernel, dim3((unsigned)((Nf + NM_WAVES - 1) / NM_WAVES)), dim3(64 * NM_WAVES),
                     0, ctx->stream, e, (long long)L, (int)hop, (int)Nf, theta, f0, (const unsigned char*)voiced,
                     (int)No_ti, ti0, step, fs, (int)harmonics, mod);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_noise_warp(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf, int32_t order,
                                const double* alpha, double* sigma_out, double* refl_out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!sigma || !refl || !alpha || !sigma_out || !refl_out || Nf < 1)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_warp: bad argument");
  if (order < 1 || order > 63) return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_warp: need 1 <= order <= 63");
  hipLaunchKernelGGL(eaqhm_noise_warp_kernel, dim3((unsigned)(((int64_t)Nf + NW_WAVES - 1) / NW_WAVES)),
                     dim3(64 * NW_WAVES), 0, ctx->stream, sigma, refl, (int)Nf, (int)order, alpha, sigma_out, refl_out);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_noise_envelope(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf, int32_t order,
                                    const double* alpha, const double* fnorm, int32_t F, double* out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!sigma || !refl || !alpha || !fnorm || !out || Nf < 1 || F < 1)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_envelope: bad argument");
  if (order < 1 || order > 63) return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_envelope: need 1 <= order <= 63");
  hipLaunchKernelGGL(eaqhm_noise_envelope_kernel, dim3((unsigned)(((int64_t)Nf + NE_WAVES - 1) / NE_WAVES)),
                     dim3(64 * NE_WAVES), 0, ctx->stream, sigma, refl, (int)Nf, (int)order, alpha, fnorm, (int)F, out);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

// ---- the piecewise-linear formant warp of the noise model; breakpoints in cycles per sample
extern "C" int eaqhm_noise_warp_map(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf, int32_t order,
                                    const double* f_in, const double* f_out, int32_t B, double* sigma_out,
                                    double* refl_out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!sigma || !refl || !f_in || !f_out || !sigma_out || !refl_out || Nf < 1)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_warp_map: bad argument");
  if (order < 1 || order > 63) return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_warp_map: need 1 <= order <= 63");
  if (B < 1 || B > WARP_BMAX) return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_warp_map: need 1 <= B <= 16 breakpoints");
  hipLaunchKernelGGL(eaqhm_noise_warp_map_kernel, dim3((unsigned)(((int64_t)Nf + NW_WAVES - 1) / NW_WAVES)),
                     dim3(64 * NW_WAVES), 0, ctx->stream, sigma, refl, (int)Nf, (int)order, f_in, f_out, (int)B, sigma_out,
                     refl_out);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_noise_envelope_map(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf,
                                        int32_t order, const double* f_in, const double* f_out, int32_t B,
                                        const double* fnorm, int32_t F, double* out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!sigma || !refl || !f_in || !f_out || !fnorm || !out || Nf < 1 || F < 1)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_envelope_map: bad argument");
  if (order < 1 || order > 63) return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_envelope_map: need 1 <= order <= 63");
  if (B < 1 || B > WARP_BMAX) return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_envelope_map: need 1 <= B <= 16 breakpoints");
  hipLaunchKernelGGL(eaqhm_noise_envelope_map_kernel, dim3((unsigned)(((int64_t)Nf + NE_WAVES - 1) / NE_WAVES)),
                     dim3(64 * NE_WAVES), 0, ctx->stream, sigma, refl, (int)Nf, (int)order, f_in, f_out, (int)B, fnorm,
                     (int)F, out);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

// ---- the noise model to and from cepstral rows
extern "C" int eaqhm_noise_cepstrum(eaqhm_ctx* ctx, const double* sigma, const double* refl, int32_t Nf, int32_t order,
                                    int32_t ceps_order, double* ceps) {
  if (!ctx) return EAQHM_EINVAL;
  if (!sigma || !refl || !ceps || Nf < 1) return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_cepstrum: bad argument");
  if (order < 1 || order > 63 || ceps_order < 1 || ceps_order > 63)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_noise_cepstrum: need 1 <= order <= 63 and 1 <= ceps_order <= 63");
  hipLaunchKernelGGL(eaqhm_noise_cepstrum_kernel, dim3((unsigned)(((int64_t)Nf + NC_WAVES - 1) / NC_WAVES)),
                     dim3(64 * NC_WAVES), 0, ctx->stream, sigma, refl, (int)Nf, (int)order, (int)ceps_order, ceps);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

static int noise_from_cepstrum_launch(eaqhm_ctx* ctx, const char* fn, const double* ceps, int32_t Nf,
                                      int32_t ceps_order, int32_t order, double* sigma_out, double* refl_out,
                                      const double* warp) {
  if (!ctx) return EAQHM_EINVAL;
  char msg[160];
  const char* what = nullptr;
  if (!ceps || !sigma_out || !refl_out || Nf < 1) what = "bad argument";
  else if (order < 1 || order > 63 || ceps_order < 1 || ceps_order > 63)
    what = "need 1 <= order <= 63 and 1 <= ceps_order <= 63";
  else if (warp && !(std::isfinite(*warp) && fabs(*warp) <= 0.9)) what = "cep_warp must be finite with |cep_warp| <= 0.9";
  if (what) {
    snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    return ctx->fail(EAQHM_EINVAL, msg);
  }
  const dim3 grid((unsigned)(((int64_t)Nf + NW_WAVES - 1) / NW_WAVES)), block(64 * NW_WAVES);
  hipLaunchKernelGGL(warp ? eaqhm_noise_from_cepstrum_kernel<true> : eaqhm_noise_from_cepstrum_kernel<false>, grid, block,
                     0, ctx->stream, ceps, (int)Nf, (int)ceps_order, (int)order, sigma_out, refl_out, warp ? *warp : 0.0);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_noise_from_cepstrum(eaqhm_ctx* ctx, const double* ceps, int32_t Nf, int32_t ceps_order,
                                         int32_t order, double* sigma_out, double* refl_out) {
  return noise_from_cepstrum_launch(ctx, "eaqhm_noise_from_cepstrum", ceps, Nf, ceps_order, order, sigma_out, refl_out,
                                    nullptr);
}
extern "C" int eaqhm_noise_from_cepstrum_warped(eaqhm_ctx* ctx, const double* ceps, int32_t Nf, int32_t ceps_order,
                                                int32_t order, double* sigma_out, double* refl_out, double cep_warp) {
  return noise_from_cepstrum_launch(ctx, "eaqhm_noise_from_cepstrum_warped", ceps, Nf, ceps_order, order, sigma_out,
                                    refl_out, &cep_warp);
}
