// eaqhm_cepstrum.hip — the discrete-cepstrum spectral envelope of an eaQHM model.  gfx950 (MI355X)
// only, FP64.  Per analysis instant order + 1 coefficients c_p of a smooth log-amplitude envelope
//   C(w) = c_0 + 2 sum_{p=1..P} c_p cos(p w),   w = 2 pi f / fs,
// fitted to the instant's partial peaks by regularised least squares (Galas & Rodet 1990; Cappe & Moulines 1996).
//
//   eaqhm_model_cepstrum_kernel<WARP> one wave per instant: the fit (nodes to LDS, the cosine sums T_d, in-wave Cholesky)
//   eaqhm_modify_amp_cepstrum_kernel  one wave per instant: the knot amplitudes A' read off a supplied cepstrum
//   eaqhm_cepstrum_envelope_kernel    one wave per row: the envelope on a frequency grid
//   eaqhm_cepstrum_phase_kernel       its sibling: the minimum-phase response Phi of the envelope on the grid (§9.7)
//   eaqhm_model_build_kernel<WARP>    one wave per instant: the records of a harmonic model from f0 and a cepstrum (§9.7)
// The readouts share cep_read: the read frequency (none, / alpha, or the inverse formant warp of eaqhm_warp.h), the hold
// outside [0, fs/2] and Clenshaw's recurrence from one cos; cep_recur gives the kernels of §9.7 the sine sum as well.
// Every kernel has a sibling (§9.8; include/eaqhm_cepwarp.h) on the all-pass warped axis Omega_a(w).  The fit and the
// build are kernel templates <bool WARP> (the body is compiled as the kernel: both instantiations keep the machine code
// they had as separate texts, tools/isa_diff.py; profilers show them under their C++ names); the readouts inline a
// shared device template into a *_kernel and a *_warped_kernel wrapper, which left their unwarped code as it was.
#include "eaqhm_common.h"
#include "eaqhm_warp.h"
#include "eaqhm_wave.h"

namespace eaqhm {

#define CEP_WAVES 4
constexpr int CEP_PMAX = 63;   // order at most: lane r of a wave owns row r of the (order + 1)-square system

// ------------------------------------------------------------------------------------------------
// The fit.  (M^T M + lambda R) c = M^T v with M[n][0] = 1, M[n][p] = 2 cos(p w_n), R = diag(8 pi^2 p^2).
// Product-to-sum makes M^T M Toeplitz + Hankel in T_d = sum_n cos(d w_n), d = 0..2P:
//   G_00 = T_0,  G_p0 = 2 T_p,  G_pq = 2 (T_|p-q| + T_{p+q}),
// so the nodes are visited (2P + 1) + (P + 1) times, not (P + 1)^2 times.
// LDS of a wave (doubles): w_n [K], v_n [K], T [2P + 2], then the lower triangle of the factor, P + 1 rows at the odd
// stride LS = (P + 1) | 1 (lane r reads its own row at r LS + j: 32 consecutive lanes hit 32 different 8-byte banks).
__host__ __device__ inline int cep_stride(int P) { return (P + 1) | 1; }
__host__ __device__ inline size_t cep_wave_doubles(int K, int P) {
  return (size_t)2 * K + (size_t)(2 * P + 2) + (size_t)(P + 1) * cep_stride(P);
}

// entry (r, q), r >= q, of M^T M + lambda R from the cosine sums
__device__ inline double cep_gram(const double* T, int r, int q, double lam) {
  if (q == 0) return r == 0 ? T[0] : 2.0 * T[r];
  double g = 2.0 * (T[r - q] + T[r + q]);
  if (r == q) g += lam * ((8.0 * M_PI * M_PI) * (double)(r * r));
  return g;
}

// The warped axis (§9.8): Omega_a(w) = w + 2 atan2(a sin w, 1 - a cos w), |a| <= 0.9.  The fit takes it as it is, once
// per node.  The readouts need only functions of Omega that are a rational map of sin and cos of w / 2: with
// u = (1 + a) sin(w/2), v = (1 - a) cos(w/2), tan(Omega/2) = u / v, so
//   cos Omega = (v - u)(v + u) / (u^2 + v^2),   sin Omega = 2 u v / (u^2 + v^2):
// one division, no atan2, and a denominator of two squares (>= (1 - |a|)^2) that cannot cancel.
struct CepAxis { double p, m; };   // 1 + a, 1 - a
__device__ inline CepAxis cep_axis(double a) { return CepAxis{1.0 + a, 1.0 - a}; }

__device__ inline double cep_omega(double a, double w) {
  double sn, cs;
  sincos(w, &sn, &cs);
  return w + 2.0 * atan2(a * sn, 1.0 - a * cs);
}

// The readouts on this axis run Clenshaw's recurrence in Reinsch's form.  Omega_a crowds a whole band towards 0 (a < 0)
// or pi (a > 0), where cos Omega, rounded once, no longer tells Omega: the plain recurrence from 2 cos Omega multiplies
// that rounding by up to p^2 (264 x the model's own float64 error at a = -0.9, P = 63, 2.3 kHz).
// Reinsch's form takes dl = -4 sin^2(Omega/2) = -4 u^2 / (u^2 + v^2) on the half cos Omega >= 0 and
// dl = 4 cos^2(Omega/2) = 4 v^2 / (u^2 + v^2) on the other, both without a subtraction; with sg = +-1 for the half,
//   d_p = c_p + dl b_{p+1} + sg d_{p+1},   b_p = d_p + sg b_{p+1}       (d_p = b_p - sg b_{p+1}),
// b_p the plain recurrence's, so  sum_p c_p cos(p Omega) = dl b_1 / 2 + sg d_1  and  sum_p c_p sin(p Omega) = b_1 sn.
struct CepAngle { double dl, sg, sn; };   // of Omega_a(w): dl and sg as above, sn = sin Omega

__device__ inline CepAngle cep_axis_angle(const CepAxis& X, double wh) {   // wh = w / 2 in [0, pi/2]: u, v >= 0
  double sh, ch;
  sincos(wh, &sh, &ch);
  const double u = X.p * sh, v = X.m * ch;
  const double uu = u * u, vv = v * v;
  const double r = 1.0 / (uu + vv);
  const bool low = vv >= uu;   // cos Omega = (v - u)(v + u) / (u^2 + v^2) >= 0
  return CepAngle{low ? -4.0 * (uu * r) : 4.0 * (vv * r), low ? 1.0 : -1.0, (2.0 * (u * v)) * r};
}

// leaves b = b_1 and d = d_1
__device__ inline void cep_recur_reinsch(const double* c, int P, const CepAngle& A, double& b, double& d) {
  b = 0.0;
  d = 0.0;
  for (int p = P; p >= 1; --p) {   // one LDS address for the wave: a broadcast
    d = c[p] + (A.dl * b + A.sg * d);
    b = d + A.sg * b;
  }
}

// WARP (§9.8): the nodes are staged at Omega_a(w_n), a = cep_a (0.0 and not read without it).
template <bool WARP>
__global__ void __launch_bounds__(64 * CEP_WAVES)
    eaqhm_model_cepstrum_kernel(const double* __restrict__ records, int No_ti, int K, double fs, int P, double lam,
                                double* __restrict__ ceps, double cep_a) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * CEP_WAVES + w);   // one wave per instant: scalar
  if (i >= No_ti) return;   // the waves of a block share no data: no block barrier below
  const int n = P + 1, LS = cep_stride(P);
  double* sw = lds + (size_t)w * cep_wave_doubles(K, P);
  double* sv = sw + K;
  double* T = sv + K;
  double* A = T + (2 * P + 2);
  const double* row = records + (size_t)i * (3 * K + 1);
  double* out = ceps + (size_t)i * n;

  // ---- 1. the nodes: the active slots (am != 0, f > 0) in slot order
  int nn = 0;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane;
    const bool act = k < K && row[k] != 0.0 && row[K + k] > 0.0;
    const unsigned long long m = __ballot(act);
    if (act) {
      const int p = nn + __popcll(m & ((1ull << lane) - 1ull));
      const double wn = ((2.0 * M_PI) * row[K + k]) / fs;
      if constexpr (WARP) sw[p] = cep_omega(cep_a, wn);
      else sw[p] = wn;
      sv[p] = log(row[k]);
    }
    nn += __popcll(m);
  }
  if (nn == 0) {   // an empty instant: -inf, 0, .., 0
    if (lane < n) out[lane] = lane == 0 ? -INFINITY : 0.0;
    return;
  }
  __builtin_amdgcn_wave_barrier();

  // ---- 2. T_d = sum_n cos(d w_n), d = 0..2P, and b_p = sum_n v_n m_p(w_n), p = 0..P: lanes over d, every lane walks
  // the nodes (one LDS address for the wave: a broadcast).  Each cosine is taken at d w_n itself, so there is no
  // phasor to drift.  d <= P <= 63 falls in the first round: b_r ends up in lane r, the owner of row r.
  double b = 0.0;
  for (int d = lane; d <= 2 * P; d += 64) {
    const double dd = (double)d;
    double t = 0.0, bv = 0.0;
    for (int q = 0; q < nn; ++q) {
      const double c = cos(dd * sw[q]);
      t += c;
      bv += sv[q] * c;
    }
    T[d] = t;
    if (d <= P) b = d == 0 ? bv : 2.0 * bv;
  }
  __builtin_amdgcn_wave_barrier();

  // ---- 3. Cholesky G = L L^T, column by column (left-looking): lane r >= j forms G_rj - sum_{k<j} L_rk L_jk from its
  // own row and row j (a broadcast); the pivot comes from lane j.  A pivot that is not finite or not > 0 ends the fit
  // with a NaN row.
  const int r = lane;
  bool bad = false;
  for (int j = 0; j < n; ++j) {
    double s = 0.0;
    if (r >= j && r < n) {
      s = cep_gram(T, r, j, lam);
      for (int k = 0; k < j; ++k) s -= A[r * LS + k] * A[j * LS + k];
    }
    const double piv = wave_lane(s, j);
    if (!(piv > 0.0) || !(piv < INFINITY)) { bad = true; break; }   // wave-uniform
    const double dj = sqrt(piv);
    if (r >= j && r < n) A[r * LS + j] = r == j ? dj : s / dj;
    __builtin_amdgcn_wave_barrier();
  }
  if (bad) {
    if (r < n) out[r] = NAN;
    return;
  }
  // forward: L y = b, column by column; lane j keeps y_j
  double y = b;
  for (int j = 0; j < n; ++j) {
    const double yj = wave_lane(y, j) / A[j * LS + j];
    if (r == j) y = yj;
    else if (r > j && r < n) y -= A[r * LS + j] * yj;
  }
  // backward: L^T c = y; lane r < j reads L_jr along row j (consecutive addresses)
  for (int j = n - 1; j >= 0; --j) {
    const double cj = wave_lane(y, j) / A[j * LS + j];
    if (r == j) y = cj;
    else if (r < j) y -= A[j * LS + r] * cj;
  }
  if (r < n) out[r] = y;
}

// ------------------------------------------------------------------------------------------------
// The readout: C(q) = c_0 + 2 sum_p c_p cos(p wq), wq = 2 pi q^ / fs, q^ = min(max(read(q), 0), fs/2) (held past
// Nyquist).  read(q) is q, q / alpha or V(q) (mode 0, 1, 2).  Clenshaw from one cos; c_0 is added last, so that the
// -inf of an empty row stays -inf.  c: the row's P + 1 coefficients (LDS).
struct CepRead { const double* c; int P; double fs; int mode; double alpha; };

// the read frequency of all four readouts, in Hz: read(q) by the mode, held at [0, fs/2]
__device__ inline double cep_read_freq(const CepRead& R, const WarpRow& W, double q) {
  const double x = R.mode == 1 ? q / R.alpha : R.mode == 2 ? warp_inverse(W, q) : q;
  return fmin(fmax(x, 0.0), 0.5 * R.fs);
}

__device__ inline double cep_read(const CepRead& R, const WarpRow& W, double q) {
  const double x = cep_read_freq(R, W, q);
  const double cw2 = 2.0 * cos(((2.0 * M_PI) * x) / R.fs);
  double b1 = 0.0, b2 = 0.0;
  for (int p = R.P; p >= 1; --p) {   // one LDS address for the wave: a broadcast
    const double b0 = R.c[p] + (cw2 * b1 - b2);
    b2 = b1;
    b1 = b0;
  }
  return 2.0 * (0.5 * cw2 * b1 - b2) + R.c[0];
}

// The same recurrence for the kernels of §9.7, which need the sine sum too: from cw2 = 2 cos(t) it leaves b_1, b_2 with
//   sum_p c_p cos(p t) = b_1 cos(t) - b_2   and   sum_p c_p sin(p t) = b_1 sin(t).
// (A helper of its own: cep_read above stays as it is, and with it the code of the kernels that use it.)
__device__ inline void cep_recur(const double* c, int P, double cw2, double& b1, double& b2) {
  b1 = 0.0;
  b2 = 0.0;
  for (int p = P; p >= 1; --p) {   // one LDS address for the wave: a broadcast
    const double b0 = c[p] + (cw2 * b1 - b2);
    b2 = b1;
    b1 = b0;
  }
}

// Phi(q) = -2 sum_p c_p sin(p wq) at the read frequency of cep_read: the minimum-phase response of the envelope; an
// empty row (every c_p = 0) reads 0.
__device__ inline double cep_read_phase(const CepRead& R, const WarpRow& W, double q) {
  const double x = cep_read_freq(R, W, q);
  double sn, cs, b1, b2;
  sincos(((2.0 * M_PI) * x) / R.fs, &sn, &cs);
  cep_recur(R.c, R.P, 2.0 * cs, b1, b2);
  return -2.0 * (b1 * sn);
}

// The two readouts on the warped axis (§9.8): the read frequency and the hold as above, in Hz, then Omega_a through
// cep_axis_angle and the recurrence in Reinsch's form.
__device__ inline double cep_read_warped(const CepRead& R, const CepAxis& X, const WarpRow& W, double q) {
  const double x = cep_read_freq(R, W, q);
  const CepAngle A = cep_axis_angle(X, (M_PI * x) / R.fs);
  double b, d;
  cep_recur_reinsch(R.c, R.P, A, b, d);
  return 2.0 * (0.5 * A.dl * b + A.sg * d) + R.c[0];
}

__device__ inline double cep_read_phase_warped(const CepRead& R, const CepAxis& X, const WarpRow& W, double q) {
  const double x = cep_read_freq(R, W, q);
  const CepAngle A = cep_axis_angle(X, (M_PI * x) / R.fs);
  double b, d;
  cep_recur_reinsch(R.c, R.P, A, b, d);
  return -2.0 * (b * A.sn);
}

// LDS of the two readout kernels (doubles): per wave the row's coefficients [CEP_PMAX + 1] and its row of the map
// [2 x WARP_BMAX], then the block's x [WARP_BMAX].  A block barrier follows the staging; every wave reaches it.
constexpr int CEP_READ_WAVE = CEP_PMAX + 1 + 2 * WARP_BMAX;
constexpr size_t CEP_READ_LDS = ((size_t)CEP_WAVES * CEP_READ_WAVE + WARP_BMAX) * sizeof(double);

__device__ inline WarpRow cep_stage(double* lds, int w, int lane, bool live, const double* __restrict__ crow, int P,
                                    const double* __restrict__ f_in, const double* __restrict__ yrow, int B) {
  double* c = lds + (size_t)w * CEP_READ_WAVE;
  double* wy = c + (CEP_PMAX + 1);
  double* ws = wy + WARP_BMAX;
  double* wx = lds + (size_t)CEP_WAVES * CEP_READ_WAVE;
  if (live && lane <= P) c[lane] = crow[lane];
  bool ident = true;
  if (B > 0) {
    warp_stage_x(f_in, B, threadIdx.x, wx);
    if (live) ident = warp_stage(f_in, yrow, B, lane, wy, ws);
  }
  __syncthreads();
  return WarpRow{wx, wy, ws, B, ident};
}

// A'[i][k] = exp(C_i(read_i(beta_i f_k))) for an active slot, 0 for an inactive one and where beta_i f_k >= fs/2.
// There is no unit rule: the envelope is the caller's.  Overwrites the amp of a prep that ran without the envelope.
template <bool WARP>
__device__ __forceinline__ void cep_amp(double* lds, const double* __restrict__ records, int No_ti, int K, double fs,
                                        const double* __restrict__ betav, const double* __restrict__ ceps, int P,
                                        const double* __restrict__ alphav, const double* __restrict__ f_in,
                                        const double* __restrict__ f_out, int B, double* __restrict__ amp, double aw) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * CEP_WAVES + w);   // one wave per instant: scalar
  const bool live = i < No_ti;
  const int il = live ? i : 0;
  const WarpRow W = cep_stage(lds, w, lane, live, ceps + (size_t)il * (P + 1), P, f_in, f_out + (size_t)il * B, B);
  if (!live) return;
  const double beta = betav[i];
  const CepRead R{lds + (size_t)w * CEP_READ_WAVE, P, fs, B > 0 ? 2 : alphav ? 1 : 0, alphav ? alphav[i] : 1.0};
  const CepAxis X = cep_axis(aw);
  const double* row = records + (size_t)i * (3 * K + 1);
  for (int k = lane; k < K; k += 64) {
    const double ak = row[k], fk = row[K + k];
    double a = 0.0;
    if (ak != 0.0 && fk > 0.0) {
      const double bf = beta * fk;   // the output frequency: it alone decides the muting
      a = exp(WARP ? cep_read_warped(R, X, W, bf) : cep_read(R, W, bf));
      if (bf >= 0.5 * fs) a = 0.0;
    }
    amp[(size_t)i * K + k] = a;
  }
}

extern "C" __global__ void __launch_bounds__(64 * CEP_WAVES)
    eaqhm_modify_amp_cepstrum_kernel(const double* __restrict__ records, int No_ti, int K, double fs,
                                     const double* __restrict__ betav, const double* __restrict__ ceps, int P,
                                     const double* __restrict__ alphav, const double* __restrict__ f_in,
                                     const double* __restrict__ f_out, int B, double* __restrict__ amp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  cep_amp<false>(lds, records, No_ti, K, fs, betav, ceps, P, alphav, f_in, f_out, B, amp, 0.0);
}

extern "C" __global__ void __launch_bounds__(64 * CEP_WAVES)
    eaqhm_modify_amp_cepstrum_warped_kernel(const double* __restrict__ records, int No_ti, int K, double fs,
                                            const double* __restrict__ betav, const double* __restrict__ ceps, int P,
                                            const double* __restrict__ alphav, const double* __restrict__ f_in,
                                            const double* __restrict__ f_out, int B, double* __restrict__ amp,
                                            double aw) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  cep_amp<true>(lds, records, No_ti, K, fs, betav, ceps, P, alphav, f_in, f_out, B, amp, aw);
}

// out[i][t] = C_i(read_i(freqs[t])), natural-log amplitude, not muted; -inf on a (-inf, 0, ..) row.  PHASE: Phi_i there.
template <bool PHASE, bool WARP = false>
__device__ inline void cep_grid(double* lds, const double* __restrict__ ceps, int n, int P, double fs,
                                const double* __restrict__ alphav, const double* __restrict__ f_in,
                                const double* __restrict__ f_out, int B, const double* __restrict__ freqs, int F,
                                double* __restrict__ out, double aw = 0.0) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * CEP_WAVES + w);   // one wave per row: scalar
  const bool live = i < n;
  const int il = live ? i : 0;
  const WarpRow W = cep_stage(lds, w, lane, live, ceps + (size_t)il * (P + 1), P, f_in, f_out + (size_t)il * B, B);
  if (!live) return;
  const CepRead R{lds + (size_t)w * CEP_READ_WAVE, P, fs, B > 0 ? 2 : alphav ? 1 : 0, alphav ? alphav[i] : 1.0};
  if (WARP) {
    const CepAxis X = cep_axis(aw);
    for (int t = lane; t < F; t += 64)
      out[(size_t)i * F + t] = PHASE ? cep_read_phase_warped(R, X, W, freqs[t]) : cep_read_warped(R, X, W, freqs[t]);
    return;
  }
  for (int t = lane; t < F; t += 64) out[(size_t)i * F + t] = PHASE ? cep_read_phase(R, W, freqs[t]) : cep_read(R, W, freqs[t]);
}

extern "C" __global__ void __launch_bounds__(64 * CEP_WAVES)
    eaqhm_cepstrum_envelope_kernel(const double* __restrict__ ceps, int n, int P, double fs,
                                   const double* __restrict__ alphav, const double* __restrict__ f_in,
                                   const double* __restrict__ f_out, int B, const double* __restrict__ freqs, int F,
                                   double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  cep_grid<false>(lds, ceps, n, P, fs, alphav, f_in, f_out, B, freqs, F, out);
}

extern "C" __global__ void __launch_bounds__(64 * CEP_WAVES)
    eaqhm_cepstrum_phase_kernel(const double* __restrict__ ceps, int n, int P, double fs,
                                const double* __restrict__ alphav, const double* __restrict__ f_in,
                                const double* __restrict__ f_out, int B, const double* __restrict__ freqs, int F,
                                double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  cep_grid<true>(lds, ceps, n, P, fs, alphav, f_in, f_out, B, freqs, F, out);
}

extern "C" __global__ void __launch_bounds__(64 * CEP_WAVES)
    eaqhm_cepstrum_envelope_warped_kernel(const double* __restrict__ ceps, int n, int P, double fs,
                                          const double* __restrict__ alphav, const double* __restrict__ f_in,
                                          const double* __restrict__ f_out, int B, const double* __restrict__ freqs,
                                          int F, double* __restrict__ out, double aw) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  cep_grid<false, true>(lds, ceps, n, P, fs, alphav, f_in, f_out, B, freqs, F, out, aw);
}

extern "C" __global__ void __launch_bounds__(64 * CEP_WAVES)
    eaqhm_cepstrum_phase_warped_kernel(const double* __restrict__ ceps, int n, int P, double fs,
                                       const double* __restrict__ alphav, const double* __restrict__ f_in,
                                       const double* __restrict__ f_out, int B, const double* __restrict__ freqs, int F,
                                       double* __restrict__ out, double aw) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  cep_grid<true, true>(lds, ceps, n, P, fs, alphav, f_in, f_out, B, freqs, F, out, aw);
}

// ------------------------------------------------------------------------------------------------
// The model from parameters (§9.7): the records [n][3 Kmax + 1] of the harmonic model with f = h f0_i, |a| = exp(C_i(f))
// and phase = wrap(2 pi frac(h theta_i) + Phi_i(f)), h = k + 1.  Slot k is active iff the instant is voiced, its row is
// not the empty row, k < Kcap, h f0_i < fs/2 (this product, as the host forms it) and exp did not underflow; every other
// cell is written as 0 by the same stores.  One sincos per cell serves C and Phi through cep_recur.  The row's
// coefficients sit in the wave's own LDS: the waves of a block share no data, so there is no block barrier.
// WARP (§9.8): the row lies on the warped axis, a = cep_a (0.0 and not read without it): the cell's angle through the
// rational map and the recurrence in Reinsch's form (cep_axis_angle).
template <bool WARP>
__global__ void __launch_bounds__(64 * CEP_WAVES)
    eaqhm_model_build_kernel(const double* __restrict__ f0, const double* __restrict__ theta,
                             const unsigned char* __restrict__ voiced, const double* __restrict__ ceps, int P,
                             const double* __restrict__ a0, int n, double fs, int Kmax, int Kcap, int zero_phase,
                             double* __restrict__ records, double cep_a) {
  __shared__ double sc[CEP_WAVES][CEP_PMAX + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * CEP_WAVES + w);   // one wave per instant: scalar
  if (i >= n) return;
  double* c = sc[w];
  if (lane <= P) c[lane] = ceps[(size_t)i * (P + 1) + lane];
  __builtin_amdgcn_wave_barrier();
  const bool rowlive = voiced[i] != 0 && c[0] != -INFINITY;
  const double fi = f0[i], th = theta[i], half = 0.5 * fs;
  double* row = records + (size_t)i * (3 * (size_t)Kmax + 1);
  for (int k0 = 0; k0 < Kmax; k0 += 64) {
    const int k = k0 + lane;
    if (k >= Kmax) break;
    const double h = (double)(k + 1);
    const double fm = __dmul_rn(h, fi);
    double a = 0.0, f = 0.0, ph = 0.0;
    if (rowlive && k < Kcap && fm < half) {
      double sn, b1;   // sin of the cell's angle and b_1 of its recurrence: Phi = -2 b_1 sn
      if constexpr (WARP) {
        double d1;
        const CepAngle A = cep_axis_angle(cep_axis(cep_a), (M_PI * fm) / fs);
        sn = A.sn;
        cep_recur_reinsch(c, P, A, b1, d1);
        a = exp(2.0 * (0.5 * A.dl * b1 + A.sg * d1) + c[0]);
      } else {
        double cs, b2;
        sincos(((2.0 * M_PI) * fm) / fs, &sn, &cs);
        const double cw2 = 2.0 * cs;
        cep_recur(c, P, cw2, b1, b2);
        a = exp(2.0 * (0.5 * cw2 * b1 - b2) + c[0]);
      }
      if (a != 0.0) {
        const double hs = __dmul_rn(h, th);           // the product rounded as the definition rounds it, then frac
        double x = __dmul_rn(2.0 * M_PI, hs - floor(hs));
        if (!zero_phase) x += -2.0 * (b1 * sn);
        ph = x - (2.0 * M_PI) * ceil((x - M_PI) / (2.0 * M_PI));   // into (-pi, pi]
        f = fm;
      }
    }
    row[k] = a;
    row[Kmax + k] = f;
    row[2 * Kmax + k] = ph;
  }
  if (lane == 0) row[3 * (size_t)Kmax] = a0[i];
}
}  // namespace eaqhm

using namespace eaqhm;

static bool finite_pos(double x) { return std::isfinite(x) && x > 0.0; }
static const size_t CEPSTRUM_LDS_MAX = 160 * 1024;
static const int BUILD_KCAP_MAX = 1706;   // the prep kernel's LDS limit on Kmax

// the optional read-frequency groups: alpha, or the whole warp group (f_in, f_out, B in [1, 16]), or neither
static bool read_group_ok(const double* alpha, const double* f_in, const double* f_out, int32_t B) {
  const bool none = !f_in && !f_out && B == 0;
  const bool whole = f_in && f_out && B >= 1 && B <= WARP_BMAX;
  return (none || whole) && !(alpha && whole);
}

// Each entry point and its *_warped sibling (include/eaqhm_cepwarp.h) share one checked launch: `warp` is null for the
// linear axis, else it points at cep_warp.  fn names the entry point in the messages.
static int cep_fail(eaqhm_ctx* ctx, const char* fn, const char* what) {
  snprintf(ctx->err, sizeof(ctx->err), "%s: %s", fn, what);
  return EAQHM_EINVAL;
}
static bool warp_ok(const double* warp) { return !warp || (std::isfinite(*warp) && fabs(*warp) <= 0.9); }
static const char* const WARP_MSG = "cep_warp must be finite with |cep_warp| <= 0.9";
static const char* const ORDER_MSG = "need 1 <= order <= 63";
static const char* const GROUP_MSG = "alpha, or f_in and f_out with 1 <= B <= 16, or neither";

static int model_cepstrum_launch(eaqhm_ctx* ctx, const char* fn, const double* records, int32_t No_ti, int32_t Kmax,
                                 double fs, int32_t order, double lambda, double* ceps, const double* warp) {
  if (!ctx) return EAQHM_EINVAL;
  if (!records || !ceps || No_ti < 1 || Kmax <= 0 || !finite_pos(fs)) return cep_fail(ctx, fn, "bad argument");
  if (order < 1 || order > CEP_PMAX) return cep_fail(ctx, fn, ORDER_MSG);
  if (!finite_pos(lambda)) return cep_fail(ctx, fn, "lambda must be finite and > 0");
  if (!warp_ok(warp)) return cep_fail(ctx, fn, WARP_MSG);
  const size_t lds = (size_t)CEP_WAVES * cep_wave_doubles(Kmax, order) * sizeof(double);
  if (lds > CEPSTRUM_LDS_MAX) return cep_fail(ctx, fn, "Kmax too large for the nodes");
  const dim3 grid((unsigned)((No_ti + CEP_WAVES - 1) / CEP_WAVES)), block(64 * CEP_WAVES);
  const auto kernel = warp ? eaqhm_model_cepstrum_kernel<true> : eaqhm_model_cepstrum_kernel<false>;
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, ctx->stream, records, (int)No_ti, (int)Kmax, fs, (int)order, lambda, ceps,
                     warp ? *warp : 0.0);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_model_cepstrum(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, double fs,
                                    int32_t order, double lambda, double* ceps) {
  return model_cepstrum_launch(ctx, "eaqhm_model_cepstrum", records, No_ti, Kmax, fs, order, lambda, ceps, nullptr);
}
extern "C" int eaqhm_model_cepstrum_warped(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, double fs,
                                           int32_t order, double lambda, double* ceps, double cep_warp) {
  return model_cepstrum_launch(ctx, "eaqhm_model_cepstrum_warped", records, No_ti, Kmax, fs, order, lambda, ceps,
                               &cep_warp);
}

static int modify_amp_cepstrum_launch(eaqhm_ctx* ctx, const char* fn, const double* records, int32_t No_ti, int32_t Kmax,
                                      double fs, const double* beta, const double* ceps, int32_t order,
                                      const double* alpha, const double* f_in, const double* f_out, int32_t B,
                                      double* amp, const double* warp) {
  if (!ctx) return EAQHM_EINVAL;
  if (!records || !beta || !ceps || !amp || No_ti < 4 || Kmax <= 0 || !finite_pos(fs))
    return cep_fail(ctx, fn, "bad argument");
  if (order < 1 || order > CEP_PMAX) return cep_fail(ctx, fn, ORDER_MSG);
  if (!read_group_ok(alpha, f_in, f_out, B)) return cep_fail(ctx, fn, GROUP_MSG);
  if (!warp_ok(warp)) return cep_fail(ctx, fn, WARP_MSG);
  const dim3 grid((unsigned)((No_ti + CEP_WAVES - 1) / CEP_WAVES)), block(64 * CEP_WAVES);
  if (warp)
    hipLaunchKernelGGL(eaqhm_modify_amp_cepstrum_warped_kernel, grid, block, CEP_READ_LDS, ctx->stream, records,
                       (int)No_ti, (int)Kmax, fs, beta, ceps, (int)order, alpha, f_in, f_out, (int)B, amp, *warp);
  else
    hipLaunchKernelGGL(eaqhm_modify_amp_cepstrum_kernel, grid, block, CEP_READ_LDS, ctx->stream, records, (int)No_ti,
                       (int)Kmax, fs, beta, ceps, (int)order, alpha, f_in, f_out, (int)B, amp);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_modify_amp_cepstrum(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, double fs,
                                         const double* beta, const double* ceps, int32_t order, const double* alpha,
                                         const double* f_in, const double* f_out, int32_t B, double* amp) {
  return modify_amp_cepstrum_launch(ctx, "eaqhm_modify_amp_cepstrum", records, No_ti, Kmax, fs, beta, ceps, order, alpha,
                                    f_in, f_out, B, amp, nullptr);
}
extern "C" int eaqhm_modify_amp_cepstrum_warped(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax,
                                                double fs, const double* beta, const double* ceps, int32_t order,
                                                const double* alpha, const double* f_in, const double* f_out,
                                                int32_t B, double* amp, double cep_warp) {
  return modify_amp_cepstrum_launch(ctx, "eaqhm_modify_amp_cepstrum_warped", records, No_ti, Kmax, fs, beta, ceps, order,
                                    alpha, f_in, f_out, B, amp, &cep_warp);
}

// the two grid readouts: phase selects Phi
static int cepstrum_grid_launch(eaqhm_ctx* ctx, const char* fn, bool phase, const double* ceps, int32_t n, int32_t order,
                                double fs, const double* alpha, const double* f_in, const double* f_out, int32_t B,
                                const double* freqs, int32_t F, double* out, const double* warp) {
  if (!ctx) return EAQHM_EINVAL;
  if (!ceps || !freqs || !out || n < 1 || F < 1 || !finite_pos(fs)) return cep_fail(ctx, fn, "bad argument");
  if (order < 1 || order > CEP_PMAX) return cep_fail(ctx, fn, ORDER_MSG);
  if (!read_group_ok(alpha, f_in, f_out, B)) return cep_fail(ctx, fn, GROUP_MSG);
  if (!warp_ok(warp)) return cep_fail(ctx, fn, WARP_MSG);
  const dim3 grid((unsigned)((n + CEP_WAVES - 1) / CEP_WAVES)), block(64 * CEP_WAVES);
  if (warp) {
    if (phase)
      hipLaunchKernelGGL(eaqhm_cepstrum_phase_warped_kernel, grid, block, CEP_READ_LDS, ctx->stream, ceps, (int)n,
                         (int)order, fs, alpha, f_in, f_out, (int)B, freqs, (int)F, out, *warp);
    else
      hipLaunchKernelGGL(eaqhm_cepstrum_envelope_warped_kernel, grid, block, CEP_READ_LDS, ctx->stream, ceps, (int)n,
                         (int)order, fs, alpha, f_in, f_out, (int)B, freqs, (int)F, out, *warp);
  } else if (phase) {
    hipLaunchKernelGGL(eaqhm_cepstrum_phase_kernel, grid, block, CEP_READ_LDS, ctx->stream, ceps, (int)n, (int)order, fs,
                       alpha, f_in, f_out, (int)B, freqs, (int)F, out);
  } else {
    hipLaunchKernelGGL(eaqhm_cepstrum_envelope_kernel, grid, block, CEP_READ_LDS, ctx->stream, ceps, (int)n, (int)order,
                       fs, alpha, f_in, f_out, (int)B, freqs, (int)F, out);
  }
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_cepstrum_envelope(eaqhm_ctx* ctx, const double* ceps, int32_t n, int32_t order, double fs,
                                       const double* alpha, const double* f_in, const double* f_out, int32_t B,
                                       const double* freqs, int32_t F, double* out) {
  return cepstrum_grid_launch(ctx, "eaqhm_cepstrum_envelope", false, ceps, n, order, fs, alpha, f_in, f_out, B, freqs, F,
                              out, nullptr);
}
extern "C" int eaqhm_cepstrum_envelope_warped(eaqhm_ctx* ctx, const double* ceps, int32_t n, int32_t order, double fs,
                                              const double* alpha, const double* f_in, const double* f_out, int32_t B,
                                              const double* freqs, int32_t F, double* out, double cep_warp) {
  return cepstrum_grid_launch(ctx, "eaqhm_cepstrum_envelope_warped", false, ceps, n, order, fs, alpha, f_in, f_out, B,
                              freqs, F, out, &cep_warp);
}
extern "C" int eaqhm_cepstrum_phase(eaqhm_ctx* ctx, const double* ceps, int32_t n, int32_t order, double fs,
                                    const double* alpha, const double* f_in, const double* f_out, int32_t B,
                                    const double* freqs, int32_t F, double* out) {
  return cepstrum_grid_launch(ctx, "eaqhm_cepstrum_phase", true, ceps, n, order, fs, alpha, f_in, f_out, B, freqs, F, out,
                              nullptr);
}
extern "C" int eaqhm_cepstrum_phase_warped(eaqhm_ctx* ctx, const double* ceps, int32_t n, int32_t order, double fs,
                                           const double* alpha, const double* f_in, const double* f_out, int32_t B,
                                           const double* freqs, int32_t F, double* out, double cep_warp) {
  return cepstrum_grid_launch(ctx, "eaqhm_cepstrum_phase_warped", true, ceps, n, order, fs, alpha, f_in, f_out, B, freqs,
                              F, out, &cep_warp);
}

static int model_build_launch(eaqhm_ctx* ctx, const char* fn, const double* f0, const double* theta,
                              const uint8_t* voiced, const double* ceps, int32_t order, const double* a0, int32_t n,
                              double fs, int32_t Kmax, int32_t Kcap, int32_t zero_phase, double* records,
                              const double* warp) {
  if (!ctx) return EAQHM_EINVAL;
  if (!f0 || !theta || !voiced || !ceps || !a0 || !records || n < 2 || !finite_pos(fs))
    return cep_fail(ctx, fn, "bad argument");
  if (order < 1 || order > CEP_PMAX) return cep_fail(ctx, fn, ORDER_MSG);
  if (Kcap < 1 || Kcap > BUILD_KCAP_MAX || Kmax < 1 || Kmax > Kcap)
    return cep_fail(ctx, fn, "need 1 <= Kmax <= Kcap <= 1706");
  if (zero_phase != 0 && zero_phase != 1) return cep_fail(ctx, fn, "zero_phase is 0 or 1");
  if (!warp_ok(warp)) return cep_fail(ctx, fn, WARP_MSG);
  const dim3 grid((unsigned)((n + CEP_WAVES - 1) / CEP_WAVES)), block(64 * CEP_WAVES);
  hipLaunchKernelGGL(warp ? eaqhm_model_build_kernel<true> : eaqhm_model_build_kernel<false>, grid, block, 0, ctx->stream,
                     f0, theta, (const unsigned char*)voiced, ceps, (int)order, a0, (int)n, fs, (int)Kmax, (int)Kcap,
                     (int)zero_phase, records, warp ? *warp : 0.0);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_model_build(eaqhm_ctx* ctx, const double* f0, const double* theta, const uint8_t* voiced,
                                 const double* ceps, int32_t order, const double* a0, int32_t n, double fs,
                                 int32_t Kmax, int32_t Kcap, int32_t zero_phase, double* records) {
  return model_build_launch(ctx, "eaqhm_model_build", f0, theta, voiced, ceps, order, a0, n, fs, Kmax, Kcap, zero_phase,
                            records, nullptr);
}
extern "C" int eaqhm_model_build_warped(eaqhm_ctx* ctx, const double* f0, const double* theta, const uint8_t* voiced,
                                        const double* ceps, int32_t order, const double* a0, int32_t n, double fs,
                                        int32_t Kmax, int32_t Kcap, int32_t zero_phase, double* records,
                                        double cep_warp) {
  return model_build_launch(ctx, "eaqhm_model_build_warped", f0, theta, voiced, ceps, order, a0, n, fs, Kmax, Kcap,
                            zero_phase, records, &cep_warp);
}
