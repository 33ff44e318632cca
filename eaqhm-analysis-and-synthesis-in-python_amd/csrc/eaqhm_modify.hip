// eaqhm_modify.hip — resynthesis from an eaQHM model with a time scale rho and a pitch scale beta.
// gfx950 (MI355X) only, FP64.  The definition is in DESIGN.md ("Resynthesis from the model"); at rho = beta = 1 it
// reproduces eaqhm_eval_kernel's synthesis (functions.py:337-385, :537-575) of the same records.
//
//   eaqhm_modify_prep_kernel   one wave per instant: the knot amplitudes A' (log-amplitude envelope of the instant's
//                              active slots, ordered in LDS, read at beta f / alpha with one binary search per slot)
//                              and the unwrapped phase increment Delta of every in-run interval that starts at the
//                              instant.  beta is per instant; the gain g_j of the contours and the
//                              formant scale alpha (§9.2) are optional.
//   eaqhm_modify_scan_kernel   segmented prefix sum of Delta along the instants of each slot (chunks of SCAN_CH
//                              instants: pass 0 chunk aggregates, pass 1 applies the carries), giving the unwrapped
//                              knot phase R and the phase of each run's first knot.
//   eaqhm_modify_carry_kernel  one wave per slot: exclusive segmented scan of the chunk aggregates (the carries).
//   eaqhm_modify_eval_kernel<CURVE, SHAPE>  blocks of output samples: the touched intervals are integrated once into
//                              LDS (as stage 1 of eaqhm_eval_kernel), then per (sample, slot) A * cos(phase), per
//                              sample the a0 spline and the sum over slots in slot order.  A kernel template, four
//                              instantiations (profilers show them under these C++ names):
//                                CURVE  the cumulative time map C of the contours in place of tau = n'/rho;
//                                SHAPE  the shape-invariant phase of DESIGN.md §11: Psi unweighted plus (k+1) times the
//                                       phase advance of the fundamental, from the per-instant tracks f0 and S.
//   eaqhm_model_envelope_kernel  reads the envelope itself out on a frequency grid.
//   eaqhm_modify_amp_warp_kernel, eaqhm_model_envelope_warp_kernel  the amplitudes A' and the readout with the
//                              piecewise-linear formant warp of DESIGN.md §9.4 (eaqhm_warp.h) in place of / alpha.
#include "eaqhm_common.h"
#include "eaqhm_pieces.h"
#include "eaqhm_warp.h"

namespace eaqhm {

struct ModArgs {
  const double* records; const unsigned char* code; const double* mom;
  int No_ti; int Kmax; int step; double fs;
};

// slot accessor straight from memory (prep kernel); make_piece reads through it
struct GSlot {
  const ModArgs& A;
  int k;
  __device__ double rec(int i, int col) const { return A.records[(size_t)i * (3 * A.Kmax + 1) + col]; }
  __device__ double fm(int i) const { return rec(i, A.Kmax + k); }
  __device__ double ph(int i) const { return rec(i, 2 * A.Kmax + k); }
  __device__ int code(int i) const { return (i < 0 || i >= A.No_ti) ? 0 : A.code[(size_t)i * A.Kmax + k]; }
  __device__ double mom(int i) const { return A.mom[(size_t)i * (A.Kmax + 1) + k]; }
};

// rows [r0, r1] of records / mom / code staged in LDS by an eval block; other rows are read from memory
struct MCache { const double* rec; const double* mom; const unsigned char* code; int r0, r1; };

struct CSlot {
  const ModArgs& A;
  const MCache& C;
  int k;
  __device__ bool in(int i) const { return i >= C.r0 && i <= C.r1; }
  __device__ double recv(int i, int col) const {
    const int RS = 3 * A.Kmax + 1;
    return in(i) ? C.rec[(size_t)(i - C.r0) * RS + col] : A.records[(size_t)i * RS + col];
  }
  __device__ double fm(int i) const { return recv(i, A.Kmax + k); }
  __device__ double ph(int i) const { return recv(i, 2 * A.Kmax + k); }
  __device__ int code(int i) const {
    if (i < 0 || i >= A.No_ti) return 0;
    return in(i) ? C.code[(size_t)(i - C.r0) * A.Kmax + k] : A.code[(size_t)i * A.Kmax + k];
  }
  __device__ double mom(int i) const {
    return in(i) ? C.mom[(size_t)(i - C.r0) * (A.Kmax + 1) + k] : A.mom[(size_t)i * (A.Kmax + 1) + k];
  }
};

// Integrated frequency of the in-run interval (j, j+1) and its closing: acc_D = sum_{v=0..D} w(v) in the eval kernel's
// order, the wrapped mismatch at the next knot and the number of whole turns Mr (functions.py:537-575).
template <class SlotT>
__device__ inline void interval_close(const SlotT& S, const FmPiece& P, int j, int D, double scale, double& w0,
                                      double& acc, double& emis, double& Mr) {
  w0 = scale * P(0);
  acc = w0;
  for (int u = 1; u <= D; ++u) acc += scale * P(u);
  const double shift = S.ph(j) - w0;
  const double e = (acc + shift) - S.ph(j + 1);
  Mr = rint(e / (2.0 * M_PI));
  emis = e - 2.0 * M_PI * Mr;
}

#define PREP_WAVES 4

// ------------------------------------------------------------------------------------------------
// Envelope nodes in LDS (eaqhm_modify_prep_kernel and eaqhm_model_envelope_kernel).  One wave per
// instant; the calls are wave-uniform and separated by a barrier:
//   env_compact  the instant's active slots (am != 0, f > 0) in slot order: their frequencies to sf[0, nn)
//   env_rank     rank of each active slot in (f, k) order, counted over sf (LDS reads only; slot order is compacted
//                order, so k breaks ties): nf[rank] = f, nv[rank] = ln am
//   env_at       E(q) on the sorted nodes: flat outside, the first of tied nodes at a node's own frequency, linear
//                between
__device__ inline int env_compact(const double* row, int K, int lane, double* sf) {
  int base = 0;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane;
    const bool act = k < K && row[k] != 0.0 && row[K + k] > 0.0;
    const unsigned long long m = __ballot(act);
    if (act) sf[base + __popcll(m & ((1ull << lane) - 1ull))] = row[K + k];
    base += __popcll(m);
  }
  return base;
}

__device__ inline void env_rank(const double* row, int K, int lane, const double* sf, int nn, double* nf,
                                double* nv) {
  int base = 0;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane;
    const bool act = k < K && row[k] != 0.0 && row[K + k] > 0.0;
    const unsigned long long m = __ballot(act);
    if (act) {
      const int p = base + __popcll(m & ((1ull << lane) - 1ull));
      const double fk = sf[p];
      int rank = 0;
      for (int q = 0; q < nn; ++q) {   // every lane reads the same sf[q]: an LDS broadcast
        const double fq = sf[q];
        rank += (fq < fk || (fq == fk && q < p)) ? 1 : 0;
      }
      nf[rank] = fk;
      nv[rank] = log(row[k]);
    }
    base += __popcll(m);
  }
}

__device__ inline double env_at(const double* nf, const double* nv, int nn, double q) {
  int lo = 0, hi = nn;   // first node with f >= q
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (nf[mid] < q) lo = mid + 1; else hi = mid;
  }
  double E;
  if (lo < nn && nf[lo] == q) E = nv[lo];
  else if (lo == 0) E = nv[0];
  else if (lo == nn) E = nv[nn - 1];
  else E = nv[lo - 1] + (nv[lo] - nv[lo - 1]) * ((q - nf[lo - 1]) / (nf[lo] - nf[lo - 1]));
  return E;
}

// ------------------------------------------------------------------------------------------------
// Envelope readout: one wave per instant i (four per block), the nodes ordered as in the prep kernel,
// lanes over the frequency grid: out[i][t] = E_i(freqs[t] / alpha_i), natural-log amplitude, not muted; -inf for an
// instant without active slots.
extern "C" __global__ void __launch_bounds__(64 * PREP_WAVES)
    eaqhm_model_envelope_kernel(const double* __restrict__ records, int No_ti, int K, const double* __restrict__ alphav,
                                const double* __restrict__ freqs, int F, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * PREP_WAVES + w;
  double* sf = lds + (size_t)w * 3 * K;
  double* nf = sf + K;
  double* nv = nf + K;
  const bool live = i < No_ti;
  const double* row = records + (size_t)(live ? i : 0) * (3 * K + 1);
  int nn = 0;
  if (live) nn = env_compact(row, K, lane, sf);
  __syncthreads();
  if (live) env_rank(row, K, lane, sf, nn, nf, nv);
  __syncthreads();
  if (!live) return;
  const double alpha = alphav[i];
  for (int t = lane; t < F; t += 64)
    out[(size_t)i * F + t] = (nn > 0) ? env_at(nf, nv, nn, freqs[t] / alpha) : -INFINITY;
}

// ------------------------------------------------------------------------------------------------
// The formant warp.  Both kernels: one wave per instant i (PREP_WAVES per block), the envelope nodes
// as above, then per wave its row of the map (eaqhm_warp.h: y_j and the slope ratios, 2 x WARP_BMAX doubles) and once
// per block x.  LDS: PREP_WAVES x 3 K doubles, then PREP_WAVES x 2 x WARP_BMAX, then WARP_BMAX.
__device__ inline WarpRow warp_row_lds(double* lds, int K, int w, int lane, bool live, const double* __restrict__ f_in,
                                       const double* __restrict__ yrow, int B) {
  double* wy = lds + (size_t)PREP_WAVES * 3 * K + (size_t)w * 2 * WARP_BMAX;
  double* ws = wy + WARP_BMAX;
  double* wx = lds + (size_t)PREP_WAVES * 3 * K + (size_t)PREP_WAVES * 2 * WARP_BMAX;
  warp_stage_x(f_in, B, threadIdx.x, wx);
  const bool ident = live ? warp_stage(f_in, yrow, B, lane, wy, ws) : true;
  return WarpRow{wx, wy, ws, B, ident};
}

// A'[i][k] = exp(E_i(V_i(beta_i f_k))) for an active slot, 0 for an inactive one and where beta_i f_k >= fs/2; an
// instant with an identity row and beta_i == 1 copies am (the prep's unit rule).  Overwrites the amp of a prep that ran
// without the envelope.
extern "C" __global__ void __launch_bounds__(64 * PREP_WAVES)
    eaqhm_modify_amp_warp_kernel(const double* __restrict__ records, int No_ti, int K, double fs,
                                 const double* __restrict__ betav, const double* __restrict__ f_in,
                                 const double* __restrict__ f_out, int B, double* __restrict__ amp) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * PREP_WAVES + w);   // one wave per instant: scalar
  double* sf = lds + (size_t)w * 3 * K;
  double* nf = sf + K;
  double* nv = nf + K;
  const bool live = i < No_ti;
  const double beta = betav[live ? i : 0];
  const double* row = records + (size_t)(live ? i : 0) * (3 * K + 1);
  const WarpRow W = warp_row_lds(lds, K, w, lane, live, f_in, f_out + (size_t)(live ? i : 0) * B, B);
  const bool unit = beta == 1.0 && W.ident;
  const bool env = live && !unit;
  int nn = 0;
  if (env) nn = env_compact(row, K, lane, sf);
  __syncthreads();
  if (env) env_rank(row, K, lane, sf, nn, nf, nv);
  __syncthreads();
  if (!live) return;
  for (int k = lane; k < K; k += 64) {
    const double ak = row[k], fk = row[K + k];
    double a = ak;
    if (!unit) {
      a = 0.0;
      if (ak != 0.0 && fk > 0.0) {
        const double bf = beta * fk;   // the output frequency: it alone decides the muting
        a = exp(env_at(nf, nv, nn, warp_inverse(W, bf)));
        if (bf >= 0.5 * fs) a = 0.0;
      }
    }
    amp[(size_t)i * K + k] = a;
  }
}

// out[i][t] = E_i(V_i(freqs[t])), natural-log amplitude, not muted; -inf for an instant without active slots
extern "C" __global__ void __launch_bounds__(64 * PREP_WAVES)
    eaqhm_model_envelope_warp_kernel(const double* __restrict__ records, int No_ti, int K,
                                     const double* __restrict__ f_in, const double* __restrict__ f_out, int B,
                                     const double* __restrict__ freqs, int F, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * PREP_WAVES + w);
  double* sf = lds + (size_t)w * 3 * K;
  double* nf = sf + K;
  double* nv = nf + K;
  const bool live = i < No_ti;
  const double* row = records + (size_t)(live ? i : 0) * (3 * K + 1);
  const WarpRow W = warp_row_lds(lds, K, w, lane, live, f_in, f_out + (size_t)(live ? i : 0) * B, B);
  int nn = 0;
  if (live) nn = env_compact(row, K, lane, sf);
  __syncthreads();
  if (live) env_rank(row, K, lane, sf, nn, nf, nv);
  __syncthreads();
  if (!live) return;
  for (int t = lane; t < F; t += 64)
    out[(size_t)i * F + t] = (nn > 0) ? env_at(nf, nv, nn, warp_inverse(W, freqs[t])) : -INFINITY;
}

// ------------------------------------------------------------------------------------------------
// Segmented scan of dR along the instants, per slot.  A segment starts at every knot whose interval to the previous
// instant is not in a run (code(i-1) == 0 or code(i) == 0).  State (sum, has_head, head phase):
//   (a) + (b) = (b.head ? b.sum : a.sum + b.sum, a.head | b.head, b.head ? b.ph : a.ph)
#define SCAN_CH 64
struct SegState { double s; double p; int h; };

__device__ inline SegState seg_combine(const SegState& a, const SegState& b) {
  SegState r;
  r.s = b.h ? b.s : a.s + b.s;
  r.p = b.h ? b.p : a.p;
  r.h = a.h | b.h;
  return r;
}

// pass 0: aggregates of every (chunk, slot) into agg[3][nchunks][K]; pass 1: R and P0 with the carry agg-scanned
// by eaqhm_modify_carry_kernel.  One thread per (chunk, slot); consecutive threads take consecutive slots (coalesced
// rows).
extern "C" __global__ void __launch_bounds__(256) eaqhm_modify_scan_kernel(const unsigned char* __restrict__ code, int No_ti,
                                                                           int K, int nchunks, int pass,
                                                                           double* __restrict__ R, double* __restrict__ P0,
                                                                           double* __restrict__ agg) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)nchunks * K) return;
  const int c = (int)(idx / K), k = (int)(idx - (long long)c * K);
  const int i0 = c * SCAN_CH, i1 = min(No_ti, i0 + SCAN_CH);
  double* aS = agg;
  double* aP = agg + (size_t)nchunks * K;
  double* aH = agg + (size_t)2 * nchunks * K;
  SegState st{0.0, 0.0, 0};
  if (pass == 1) {   // exclusive carry of this chunk (written over the aggregates by the carry kernel)
    st.s = aS[(size_t)c * K + k]; st.p = aP[(size_t)c * K + k]; st.h = aH[(size_t)c * K + k] != 0.0;
  }
  int cprev = (i0 > 0) ? code[(size_t)(i0 - 1) * K + k] : 0;
  for (int i = i0; i < i1; ++i) {
    const int ci = code[(size_t)i * K + k];
    SegState x;
    x.h = !(cprev != 0 && ci != 0);
    x.s = x.h ? 0.0 : R[(size_t)i * K + k];
    x.p = x.h ? P0[(size_t)i * K + k] : 0.0;
    st = seg_combine(st, x);
    if (pass == 1) {
      const bool run = ci != 0 && (cprev != 0 || (i + 1 < No_ti && code[(size_t)(i + 1) * K + k] != 0));
      R[(size_t)i * K + k] = run ? st.s : 0.0;
      P0[(size_t)i * K + k] = run ? st.p : 0.0;
    }
    cprev = ci;
  }
  if (pass == 0) {
    aS[(size_t)c * K + k] = st.s; aP[(size_t)c * K + k] = st.p; aH[(size_t)c * K + k] = (double)st.h;
  }
}

// one wave per slot: exclusive segmented scan of the chunk aggregates, tiles of 64 chunks with a running carry
extern "C" __global__ void __launch_bounds__(256) eaqhm_modify_carry_kernel(int K, int nchunks, double* __restrict__ agg) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= K) return;
  double* aS = agg;
  double* aP = agg + (size_t)nchunks * K;
  double* aH = agg + (size_t)2 * nchunks * K;
  SegState carry{0.0, 0.0, 0};
  for (int t0 = 0; t0 < nchunks; t0 += 64) {
    const int c = t0 + lane;
    SegState x{0.0, 0.0, 0};
    if (c < nchunks) { x.s = aS[(size_t)c * K + k]; x.p = aP[(size_t)c * K + k]; x.h = aH[(size_t)c * K + k] != 0.0; }
    SegState inc = x;   // inclusive scan inside the tile (Hillis-Steele over the wave)
    for (int o = 1; o < 64; o <<= 1) {
      SegState y;
      y.s = __shfl_up(inc.s, o); y.p = __shfl_up(inc.p, o); y.h = __shfl_up(inc.h, o);
      if (lane >= o) inc = seg_combine(y, inc);
    }
    SegState ex;
    ex.s = __shfl_up(inc.s, 1); ex.p = __shfl_up(inc.p, 1); ex.h = __shfl_up(inc.h, 1);
    ex = (lane == 0) ? carry : seg_combine(carry, ex);
    if (c < nchunks) { aS[(size_t)c * K + k] = ex.s; aP[(size_t)c * K + k] = ex.p; aH[(size_t)c * K + k] = (double)ex.h; }
    SegState last;
    last.s = __shfl(inc.s, 63); last.p = __shfl(inc.p, 63); last.h = __shfl(inc.h, 63);
    carry = seg_combine(carry, last);
  }
}

// ------------------------------------------------------------------------------------------------
// Prep: one wave per instant i (PREP_WAVES per block), 3 Kmax doubles of LDS per wave.  beta: [No_ti]; gain: [No_ti-1]
// g_j of interval j, or null (Delta unweighted); alphav: [No_ti], or null (alpha = 1).
//   A'[i][k]  beta_i == 1 and alpha_i == 1: am.  Otherwise 0 for an inactive slot and, for an active one, with the
//             envelope exp(E_i(beta_i f / alpha_i)) where E_i interpolates ln am linearly over the instant's active
//             slots sorted by (f, k) (flat outside, the first of tied nodes at a node's own frequency), without it am;
//             both muted where beta_i f >= fs/2.
//   dR[i+1][k] Delta of the interval (i, i+1) when it is in a run: (ph_{i+1} - ph_i) + 2 pi Mr, times g_i when gain is
//             given.  Other rows 0.
//   P0[i][k]  ph_i at the first knot of a run (code != 0, previous instant inactive), else 0.
// The nodes are built only where they are read; every wave of a block reaches both barriers.  The instant is a scalar
// (beta, alpha and gain come through the scalar cache) and the Delta loop, which needs none of them but gain, runs
// ahead of the barriers: the path that builds no envelope then pays for the two barriers alone.
extern "C" __global__ void __launch_bounds__(64 * PREP_WAVES)
    eaqhm_modify_prep_kernel(ModArgs A, const double* __restrict__ betav, const double* __restrict__ gain,
                             const double* __restrict__ alphav, int envelope, double* __restrict__ amp,
                             double* __restrict__ dR, double* __restrict__ P0) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int K = A.Kmax, D = A.step, RS = 3 * K + 1;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * PREP_WAVES + w);   // one wave per instant: scalar
  double* sf = lds + (size_t)w * 3 * K;   // active slots' frequencies in slot order [K], then the sorted nodes
  double* nf = sf + K;
  double* nv = nf + K;
  const bool live = i < A.No_ti;
  const double beta = betav[live ? i : 0];   // wave-uniform: one wave per instant
  const double alpha = alphav ? alphav[live ? i : 0] : 1.0;
  const double* row = A.records + (size_t)(live ? i : 0) * RS;
  const bool unit = beta == 1.0 && alpha == 1.0;
  const bool env = live && envelope && !unit;
  if (live) {
    // ---- Delta of the interval (i, i+1), first-knot phase
    const double scale = 2.0 * M_PI / A.fs;
    for (int k = lane; k < K; k += 64) {
      GSlot S{A, k};
      const int ci = S.code(i);
      const bool head = ci != 0 && S.code(i - 1) == 0;
      P0[(size_t)i * K + k] = (head && ci != 1) ? S.ph(i) : 0.0;
      if (i == 0) dR[k] = 0.0;
      if (i + 1 < A.No_ti) {
        double d = 0.0;
        if (ci != 0 && S.code(i + 1) != 0) {
          const FmPiece P = make_piece(S, i, ci);
          double w0, acc, emis, Mr;
          interval_close(S, P, i, D, scale, w0, acc, emis, Mr);
          d = (S.ph(i + 1) - S.ph(i)) + 2.0 * M_PI * Mr;
          if (gain) d = gain[i] * d;
        }
        dR[(size_t)(i + 1) * K + k] = d;
      }
    }
  }
  int nn = 0;
  if (env) nn = env_compact(row, K, lane, sf);
  __syncthreads();
  if (env) env_rank(row, K, lane, sf, nn, nf, nv);
  __syncthreads();
  if (!live) return;
  // ---- A'
  for (int k = lane; k < K; k += 64) {
    const double ak = row[k], fk = row[K + k];
    double a = ak;
    if (!unit) {
      a = 0.0;
      if (ak != 0.0 && fk > 0.0) {
        const double bf = beta * fk;   // the output frequency: it alone decides the muting
        a = envelope ? exp(env_at(nf, nv, nn, bf / alpha)) : ak;
        if (bf >= 0.5 * A.fs) a = 0.0;
      }
    }
    amp[(size_t)i * K + k] = a;
  }
}

// ------------------------------------------------------------------------------------------------
// Output sample n -> tau = n / rho, interval j = floor(tau / D) and r = tau - j D in [0, D) (the guards catch a quotient
// that rounded across an integer)
__device__ inline void locate(long long n, double rho, int D, int& j, double& r) {
  const double tau = (double)n / rho;
  const double dd = (double)D;
  double q = floor(tau / dd);
  r = tau - q * dd;
  if (r < 0.0) { q -= 1.0; r = tau - q * dd; }
  else if (r >= dd) { q += 1.0; r = tau - q * dd; }
  j = (int)q;
}

struct MEvalArgs {
  ModArgs M;
  const double* amp; const double* R; const double* P0;
  double rho; double beta; long long t_lo; long long t_hi; double* out;
};

// The contour time map of DESIGN.md §9.1: output knots C_j (C_0 = 0, C_{j+1} = C_j + r_j D), rate r_j per interval
// (the last entry is rho_{n-1}, past the last knot) and phase weight g_j per interval.
struct MCurve { const double* C; const double* rate; const double* gain; };

// The contour map as the eval kernel sees it (R holds the weighted phase G, the phase weight g_j is per interval): where
// a sample lies (locate; bound and stage prepare a block: the staged rows [NR][3] (C_j, r_j, g_j) follow the codes in
// LDS), the isolated knots of a sample (iso_range) and tau for the a0 spline.
struct CurveMap {
  MCurve G;
  int last;          // No_ti - 1
  int dstep;         // D
  int jb0, jb1;      // search bounds of the block's in-map samples
  const double* cx;  // staged rows [r0, r1] of (C_j, r_j, g_j)
  int r0, r1;
  __device__ bool in(int i) const { return i >= r0 && i <= r1; }
  __device__ double Cv(int i) const { return in(i) ? cx[(size_t)(i - r0) * 3] : G.C[i]; }
  __device__ double gv(int i) const { return in(i) ? cx[(size_t)(i - r0) * 3 + 2] : G.gain[i]; }
  // j = max{j : C_j <= n'} and r = (n' - C_j) / r_j (clamped below D); past the last knot j = last, r unbounded
  __device__ void locate(long long n, int D, int& j, double& r) const {
    const double x = (double)n;
    if (x >= G.C[last]) { j = last; r = (x - G.C[last]) / G.rate[last]; return; }
    int lo = jb0, hi = jb1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (G.C[mid] <= x) lo = mid; else hi = mid - 1;
    }
    j = lo;
    r = (x - G.C[j]) / G.rate[j];
    const double dd = (double)D;
    if (r >= dd) r = nextafter(dd, 0.0);
  }
  __device__ void bound(int jfirst, int jlast, int No_ti) { jb0 = min(jfirst, No_ti - 2); jb1 = min(jlast, No_ti - 2); }
  __device__ void stage(double* lds_rows, int rs0, int rs1, int tid, int nthr) {
    cx = lds_rows; r0 = rs0; r1 = rs1;
    const int nrow = r1 - r0 + 1;
    for (int q = tid; q < nrow * 3; q += nthr) {
      const int i = r0 + q / 3, c = q - (q / 3) * 3;
      lds_rows[q] = (c == 0) ? G.C[i] : (c == 1) ? G.rate[i] : (i < last ? G.gain[i] : 0.0);
    }
  }
  // every knot with rint(C_i) == n' lies in [n' - 0.5, n' + 0.5]: walk out from the sample's interval (several knots
  // can share one sample when r_j D < 1)
  __device__ void iso_range(long long n, int j, int No_ti, int& ilo, int& ihi) const {
    const double lo = (double)n - 0.5, hi = (double)n + 0.5;
    ilo = j;
    while (ilo > 0 && Cv(ilo - 1) >= lo) --ilo;
    ihi = j;
    while (ihi + 1 < No_ti && Cv(ihi + 1) <= hi) ++ihi;
  }
  __device__ double tau(int j, double r) const { return (double)j * (double)dstep + r; }
};


// The shape-invariant phase mode of DESIGN.md §11: the fundamental track f0_i (Hz) and its phase advance S_i (cycles,
// in [0, 1)) per instant.  Inside interval j <= No_ti - 2 at offset r the advance is s = S_j + (g_j - 1) (f0_j r +
// (f0_{j+1} - f0_j) r^2 / (2 D)) / fs, the same for every slot: stage 0 forms it once per sample, as S_j + r (c1 + r c2),
// and stage 2 adds 2 pi (k+1) s to the phase of each slot before the cosines.  Past the last knot no slot is in a run: S_{n-1} serves.
struct MShape { const double* f0; const double* S; };

__device__ inline double shape_advance(const MShape& Sh, int j, double r, double gm1, int D, double fs) {
  const double sf = Sh.f0[j], sgm = gm1 / fs;
  return Sh.S[j] + r * (sgm * sf + r * (sgm * (Sh.f0[j + 1] - sf) / (2.0 * (double)D)));
}

// ------------------------------------------------------------------------------------------------
// The eval kernel, one body for its four instantiations: CURVE picks the time map (tau = n'/rho with the phase weight
// beta rho, §9; or CurveMap with g_j per interval, §9.1) and SHAPE the shape-invariant phase term (§11).  The kernel itself is the template, so each instantiation is compiled as a
// kernel of its own; the same body inlined into four extern "C" wrappers cost the scalar one an occupancy step (§9.1).
// Cu is read only with CURVE and Sh only with SHAPE.
// Block of TBS consecutive output samples x all slots.
//   stage 0  per sample: interval j and offset r (LDS); with SHAPE also the fundamental's phase advance s(n') in
//            cycles (§11), one more double per sample after the map's staged rows.
//   stage 1  one thread per (interval, slot) touching the block: the interval's local phase
//            Psi(u) = R_j + sum_{v=1..u} w(v) - sum_{v=0..u} sin(pi v/D) er, u = 0..D, in the eval kernel's summation
//            order; at each of the block's samples in the interval the phase P0 + beta rho ((1-fr) Psi(u0) + fr Psi(u0+1))
//            goes to X[k][s].  A run's last knot (tau = c_b) is the end u = D of its last interval.  With SHAPE Psi
//            weighs 1 (§11).
//   stage 2  one thread per (sample, slot group): amplitude, A cos(phase), isolated knots (with SHAPE 2 pi (k+1) s(n')
//            is first added to the phases of the thread's cells); then one thread per sample adds the slots in slot
//            order and the a0 spline.
template <bool CURVE, bool SHAPE>
__global__ void __launch_bounds__(256) eaqhm_modify_eval_kernel(MEvalArgs E, MCurve Cu, MShape Sh, int TBS, int NR) {
  constexpr int CROW = CURVE ? 3 : 0;   // doubles per staged row that the time map adds
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const ModArgs& A = E.M;
  const int D = A.step, K = A.Kmax, TP = TBS + 1;
  double* ft = lds;                                   // D+1
  double* X = lds + ((D + 1 + 1) & ~1);               // [K][TP]
  double* sr = X + (size_t)K * TP;                    // [TBS] r of each sample
  double* crec = sr + TBS;                            // [NR][3K+1]
  double* cmom = crec + (size_t)NR * (3 * K + 1);     // [NR][K+1]
  int* sj = (int*)(cmom + (size_t)NR * (K + 1));      // [TBS] interval of each sample
  unsigned char* ccode = (unsigned char*)(sj + ((TBS + 1) & ~1));   // [NR][K]
  double* crow = (double*)(ccode + (((size_t)NR * K + 7) & ~(size_t)7));   // [NR][CROW] the map's staged rows
  double* ss = crow + (size_t)NR * CROW;              // [TBS] s of each sample (SHAPE)
  const int tid = threadIdx.x;
  const long long t0 = E.t_lo + (long long)blockIdx.x * TBS;
  const long long t1 = (t0 + TBS < E.t_hi) ? (t0 + TBS) : E.t_hi;
  const int ns = (int)(t1 - t0);
  CurveMap Mp{Cu, A.No_ti - 1, D, 0, A.No_ti - 2, nullptr, 0, -1};   // CURVE only
  auto locate_n = [&](long long n, int& j, double& r) {
    if constexpr (CURVE) Mp.locate(n, D, j, r);
    else locate(n, E.rho, D, j, r);
  };
  int jfirst, jlast;
  double rdummy;
  locate_n(t0, jfirst, rdummy);
  locate_n(t1 - 1, jlast, rdummy);
  if constexpr (CURVE) Mp.bound(jfirst, jlast, A.No_ti);
  // intervals met by the block: one before the first sample's (a run's last knot) up to the last sample's
  const int jlo = max(0, jfirst - 1), jhi = min(A.No_ti - 2, jlast);
  MCache C;
  {
    C.r0 = max(0, jlo - 1);
    C.r1 = min(A.No_ti - 1, jhi + 2);
    if (C.r1 > C.r0 + NR - 1) C.r1 = C.r0 + NR - 1;
    if (C.r1 < C.r0) C.r1 = C.r0 - 1;
    C.rec = crec; C.mom = cmom; C.code = ccode;
    const int nrow = C.r1 - C.r0 + 1, RS = 3 * K + 1;
    for (int q = tid; q < nrow * RS; q += blockDim.x) crec[q] = A.records[(size_t)C.r0 * RS + q];
    for (int q = tid; q < nrow * (K + 1); q += blockDim.x) cmom[q] = A.mom[(size_t)C.r0 * (K + 1) + q];
    for (int q = tid; q < nrow * K; q += blockDim.x) ccode[q] = A.code[(size_t)C.r0 * K + q];
    if constexpr (CURVE) Mp.stage(crow, C.r0, C.r1, tid, blockDim.x);
  }
  for (int u = tid; u <= D; u += blockDim.x) ft[u] = sin(M_PI * (double)u / (double)D);
  for (int s = tid; s < ns; s += blockDim.x) {
    int j; double r;
    locate_n(t0 + s, j, r);
    sj[s] = j; sr[s] = r;
    if constexpr (SHAPE)   // g_j from memory: the staged rows are not visible before the barrier
      ss[s] = (j < A.No_ti - 1) ? shape_advance(Sh, j, r, (CURVE ? Cu.gain[j] : E.beta * E.rho) - 1.0, D, A.fs)
                                : Sh.S[A.No_ti - 1];
  }
  __syncthreads();
  const double bw = E.beta * E.rho;   // the scalar map's phase weight, one for the block
  // ---- stage 1
  if (jhi >= jlo) {
    const int nint = jhi - jlo + 1;
    const double scale = 2.0 * M_PI / A.fs;
    double S = 0.0;   // sum_{v=0..D} sin(pi v/D), in order
    for (int u = 0; u <= D; ++u) S += ft[u];
    for (int p = tid; p < nint * K; p += blockDim.x) {
      const int jj = p / K, k = p - jj * K, j = jlo + jj;
      CSlot Sl{A, C, k};
      const int cj = Sl.code(j);
      if (cj == 0 || Sl.code(j + 1) == 0) continue;
      // the block's samples in this interval: [sa, sb), plus the run's last knot when j+1 ends the run
      int sa = 0, hi = ns;
      while (sa < hi) { const int mid = (sa + hi) >> 1; if (sj[mid] < j) sa = mid + 1; else hi = mid; }
      int sb = sa;
      while (sb < ns && sj[sb] == j) ++sb;
      const bool ends = Sl.code(j + 2) == 0;
      const int sl = (ends && sb < ns && sj[sb] == j + 1 && sr[sb] == 0.0) ? sb : -1;
      if (sa == sb && sl < 0) continue;
      const FmPiece P = make_piece(Sl, j, cj);
      double w0, acc, emis, Mr;
      interval_close(Sl, P, j, D, scale, w0, acc, emis, Mr);
      // a run's last interval closes its mismatch completely: the model's phase at that knot is the integrated one
      const double er = ends ? emis / S : M_PI * emis / (2.0 * (double)D);
      const double Rj = E.R[(size_t)j * K + k], ph0 = E.P0[(size_t)j * K + k];
      // the phase is P0 + g (R_j + local) under the scalar map and, R holding the weighted phase, (P0 + R_j) + g_j local
      // under the contours: a sum is not to be reordered, so the two add R_j at different places
      const double br = SHAPE ? 1.0 : CURVE ? Mp.gv(j) : bw, o = CURVE ? ph0 + Rj : ph0;
      acc = w0;
      double c = ft[0] * er;
      double prev = CURVE ? ((acc - w0) - c) : Rj + ((acc - w0) - c);
      int q = sa;
      // u = 0: samples on the knot itself
      while (q < sb && sr[q] == 0.0) { X[(size_t)k * TP + q] = o + br * prev; ++q; }
      for (int u = 1; u <= D; ++u) {
        acc += scale * P(u);
        c += ft[u] * er;
        const double psi = CURVE ? ((acc - w0) - c) : Rj + ((acc - w0) - c);
        while (q < sb) {
          const double rq = sr[q], u0 = floor(rq), fr = rq - u0;
          if ((int)u0 == u - 1 && fr > 0.0) X[(size_t)k * TP + q] = o + br * ((1.0 - fr) * prev + fr * psi);
          else if ((int)u0 == u && fr == 0.0) X[(size_t)k * TP + q] = o + br * psi;
          else break;
          ++q;
        }
        prev = psi;
      }
      if (sl >= 0) X[(size_t)k * TP + sl] = o + br * prev;
    }
  }
  __syncthreads();
  // ---- stage 2
  const int s = tid % TBS, g = tid / TBS, G = blockDim.x / TBS;
  const bool live = s < ns;
  const long long n = t0 + s;
  if (live) {
    const int j = sj[s];
    const double r = sr[s];
    int ilo, ihi;   // the instants whose isolated knot can land on this sample
    if constexpr (CURVE) {
      Mp.iso_range(n, j, A.No_ti, ilo, ihi);
    } else {
      const double tau = (double)n / E.rho;
      const double hw = 0.5 / E.rho + 1.0;
      ilo = max(0, (int)floor((tau - hw) / (double)D));
      ihi = min(A.No_ti - 1, (int)floor((tau + hw) / (double)D) + 1);
    }
    if constexpr (SHAPE) {
      const double shs = ss[s];
      for (int k = g; k < K; k += G) X[(size_t)k * TP + s] += (2.0 * M_PI * (double)(k + 1)) * shs;
    }
    for (int k = g; k < K; k += G) {
      CSlot Sl{A, C, k};
      auto inrun = [&](int q) { return q >= 0 && q <= A.No_ti - 2 && Sl.code(q) != 0 && Sl.code(q + 1) != 0; };
      double cell = 0.0;
      int jj = -1;
      double rr = r;
      if (inrun(j)) jj = j;
      else if (r == 0.0 && inrun(j - 1)) { jj = j - 1; rr = (double)D; }
      if (jj >= 0) {
        const double a0v = E.amp[(size_t)jj * K + k], a1v = E.amp[(size_t)(jj + 1) * K + k];
        const double Av = ((a1v - a0v) / (double)D) * rr + a0v;
        cell = (Av != 0.0) ? Av * cos(X[(size_t)k * TP + s]) : 0.0;
      }
      for (int i = ilo; i <= ihi; ++i) {   // isolated accepted knots land on the output sample nearest to their image
        if (Sl.code(i) == 1 && (long long)rint(CURVE ? Mp.Cv(i) : E.rho * ((double)i * (double)D)) == n)
          cell += E.amp[(size_t)i * K + k] * cos(Sl.ph(i));
      }
      X[(size_t)k * TP + s] = cell;   // this thread is the only reader of the cell
    }
  }
  __syncthreads();
  if (tid < TBS && live) {
    double synth = 0.0;
#pragma unroll 8
    for (int k = 0; k < K; ++k) synth += X[(size_t)k * TP + s];
    const double tau = CURVE ? Mp.tau(sj[s], sr[s]) : (double)n / E.rho;
    int ia = sj[s];
    if (ia > A.No_ti - 2) ia = A.No_ti - 2;
    if (ia < 0) ia = 0;
    CSlot S0{A, C, K};   // column K of mom = the a0 spline; its knots are the last record column
    const int RS = 3 * K + 1;
    const double a0v = spline_piece(S0.recv(ia, RS - 1), S0.recv(ia + 1, RS - 1), S0.mom(ia), S0.mom(ia + 1),
                                    tau - (double)ia * (double)D, (double)D);
    E.out[n] = a0v + 2.0 * synth;
  }
}
}  // namespace eaqhm

using namespace eaqhm;

static bool finite_pos(double x) { return std::isfinite(x) && x > 0.0; }
static int modify_scan(eaqhm_ctx* ctx, const uint8_t* code, int32_t No_ti, int32_t Kmax, double* R, double* ph0);

// LDS of the prep and envelope kernels: staged frequencies, sorted frequencies and log amplitudes per wave
static size_t envelope_lds_bytes(int Kmax) { return (size_t)PREP_WAVES * 3 * Kmax * sizeof(double); }
static const size_t ENVELOPE_LDS_MAX = 160 * 1024;

extern "C" int eaqhm_modify_prep(eaqhm_ctx* ctx, const double* records, const uint8_t* code, const double* mom,
                                 int32_t No_ti, int32_t Kmax, int32_t step, double fs, const double* beta,
                                 const double* gain, const double* alpha, int32_t preserve_envelope, double* amp,
                                 double* R, double* ph0) {
  if (!ctx) return EAQHM_EINVAL;
  if (!records || !code || !mom || !beta || !amp || !R || !ph0 || No_ti < 4 || Kmax <= 0 || step <= 0 || !finite_pos(fs))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_prep: bad argument");
  if (alpha && !preserve_envelope)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_prep: a formant scale needs the envelope (preserve_envelope != 0)");
  const size_t lds = envelope_lds_bytes(Kmax);
  if (lds > ENVELOPE_LDS_MAX) return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_prep: Kmax too large for the envelope nodes");
  const ModArgs A{records, code, mom, No_ti, Kmax, step, fs};
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_modify_prep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(eaqhm_modify_prep_kernel, dim3((unsigned)((No_ti + PREP_WAVES - 1) / PREP_WAVES)), dim3(64 * PREP_WAVES),
                     lds, ctx->stream, A, beta, gain, alpha, (int)(preserve_envelope != 0), amp, R, ph0);
  HIP_TRY(ctx, hipGetLastError());
  return modify_scan(ctx, code, No_ti, Kmax, R, ph0);
}

// the segmented scan of dR (scan pass 0, carry, scan pass 1) into R and ph0
static int modify_scan(eaqhm_ctx* ctx, const uint8_t* code, int32_t No_ti, int32_t Kmax, double* R, double* ph0) {
  const int nchunks = (No_ti + SCAN_CH - 1) / SCAN_CH;
  const size_t agg_bytes = (size_t)3 * nchunks * Kmax * sizeof(double);
  if (int rc = ctx->reserve(agg_bytes)) return rc;
  double* agg = (double*)ctx->scratch;
  const unsigned sblocks = (unsigned)(((long long)nchunks * Kmax + 255) / 256);
  hipLaunchKernelGGL(eaqhm_modify_scan_kernel, dim3(sblocks), dim3(256), 0, ctx->stream, code, No_ti, Kmax, nchunks, 0, R,
                     ph0, agg);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(eaqhm_modify_carry_kernel, dim3((unsigned)((Kmax + 3) / 4)), dim3(256), 0, ctx->stream, Kmax, nchunks,
                     agg);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(eaqhm_modify_scan_kernel, dim3(sblocks), dim3(256), 0, ctx->stream, code, No_ti, Kmax, nchunks, 1, R,
                     ph0, agg);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

// samples per block of eaqhm_modify_eval_kernel and staged rows: the largest of 64/32/16 whose tables fit; the staged
// rows follow the block's tau-span (TBS / rho samples), capped by the LDS budget (rows beyond it are read from memory).
// The contour kernel's staged rows also hold C_j, r_j, g_j (crow = 3 doubles per row; 0 for the scalar kernel); the
// shape kernels keep one more double per sample (shape = 1).
static size_t modify_lds_bytes(int K, int step, int tbs, int nr, int crow, int shape) {
  return (((size_t)step + 2) & ~(size_t)1) * 8 + (size_t)K * (tbs + 1) * 8 + (size_t)tbs * 8 +
         (size_t)nr * ((3 * (size_t)K + 1) + (K + 1)) * 8 + (((size_t)tbs + 1) & ~(size_t)1) * 4 +
         (((size_t)nr * K + 7) & ~(size_t)7) + (size_t)nr * crow * 8 + (size_t)tbs * shape * 8;
}

// rho: the smallest rate of the time map (the contour's fewest output samples per knot interval)
static int modify_block_samples(int Kmax, int step, double rho, int crow, int shape, size_t* lds_bytes, int* nr) {
  for (int tbs = 64; tbs >= 16; tbs >>= 1) {
    int NR = (int)ceil((double)(tbs - 1) / (rho * (double)step)) + 6;
    while (NR > 4 && modify_lds_bytes(Kmax, step, tbs, NR, crow, shape) > 78 * 1024) --NR;
    const size_t bytes = modify_lds_bytes(Kmax, step, tbs, NR, crow, shape);
    if (bytes <= 78 * 1024 || tbs == 16) {
      *lds_bytes = bytes; *nr = NR;
      return tbs;
    }
  }
  return 16;
}

// one eval launch: the instantiation's LDS limit, the launch, the error check
static int modify_eval_launch(eaqhm_ctx* ctx, void (*kernel)(MEvalArgs, MCurve, MShape, int, int), long long nblocks,
                              size_t lds_bytes, const MEvalArgs& E, const MCurve& Cu, const MShape& Sh, int TBS, int NR) {
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipLaunchKernelGGL(kernel, dim3((unsigned)nblocks), dim3(256), lds_bytes, ctx->stream, E, Cu, Sh, TBS, NR);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

// The time map is the contours'  when C, rate and gain are given, else tau = n'/rho; the phase is the
// shape-invariant one (§11; the prep ran without gain) when f0 and S are given, else each slot's own.  Two groups, the
// four instantiations of one kernel.
extern "C" int eaqhm_modify_synth(eaqhm_ctx* ctx, const double* records, const uint8_t* code, const double* mom,
                                  const double* amp, const double* R, const double* ph0, int32_t No_ti, int32_t Kmax,
                                  int32_t step, double fs, double rho, double beta, int64_t L_out, int64_t t_lo,
                                  int64_t t_hi, double* out, const double* C, const double* rate, const double* gain,
                                  double rate_min, const double* f0, const double* S) {
  if (!ctx) return EAQHM_EINVAL;
  const bool curve = C && rate && gain, shape = f0 && S;
  if (!records || !code || !mom || !amp || !R || !ph0 || !out || No_ti < 4 || Kmax <= 0 || step <= 0 ||
      !finite_pos(fs) || (!curve && (C || rate || gain)) || (!shape && (f0 || S)))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_synth: bad argument");
  if (curve) {   // rho and beta are not read: the kernel gets 0, 0
    if (!finite_pos(rate_min)) return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_synth: rate_min must be finite and > 0");
    rho = beta = 0.0;
  } else if (!finite_pos(rho) || !finite_pos(beta)) {
    return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_synth: rho and beta must be finite and > 0");
  }
  if (L_out <= 0 || t_lo < 0 || t_hi > L_out || t_lo >= t_hi)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_synth: [t_lo, t_hi) outside [0, L_out)");
  size_t lds_bytes = 0;
  int NR = 0;
  const int TBS = modify_block_samples(Kmax, step, curve ? rate_min : rho, curve ? 3 : 0, shape ? 1 : 0, &lds_bytes, &NR);
  if (lds_bytes > 160 * 1024) return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_synth: Kmax too large for the LDS tables");
  const MEvalArgs E{ModArgs{records, code, mom, No_ti, Kmax, step, fs}, amp, R, ph0, rho, beta, (long long)t_lo,
                    (long long)t_hi, out};
  const MCurve Cu{C, rate, gain};
  const MShape Sh{f0, S};
  const long long nblocks = (t_hi - t_lo + TBS - 1) / TBS;
  const auto kernel = curve ? (shape ? eaqhm_modify_eval_kernel<true, true> : eaqhm_modify_eval_kernel<true, false>)
                            : (shape ? eaqhm_modify_eval_kernel<false, true> : eaqhm_modify_eval_kernel<false, false>);
  return modify_eval_launch(ctx, kernel, nblocks, lds_bytes, E, Cu, Sh, TBS, NR);
}

// ---- envelope readout
extern "C" int eaqhm_model_envelope(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax,
                                    const double* alpha, const double* freqs, int32_t F, double* out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!records || !alpha || !freqs || !out || No_ti < 4 || Kmax <= 0 || F <= 0)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_model_envelope: bad argument");
  const size_t lds = envelope_lds_bytes(Kmax);
  if (lds > ENVELOPE_LDS_MAX) return ctx->fail(EAQHM_EINVAL, "eaqhm_model_envelope: Kmax too large for the envelope nodes");
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_model_envelope_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  hipLaunchKernelGGL(eaqhm_model_envelope_kernel, dim3((unsigned)((No_ti + PREP_WAVES - 1) / PREP_WAVES)),
                     dim3(64 * PREP_WAVES), lds, ctx->stream, records, (int)No_ti, (int)Kmax, alpha, freqs, (int)F, out);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

// ---- the piecewise-linear formant warp: amplitudes after a prep without the envelope, and the readout
static size_t warp_lds_bytes(int Kmax) {
  return envelope_lds_bytes(Kmax) + ((size_t)PREP_WAVES * 2 * WARP_BMAX + WARP_BMAX) * sizeof(double);
}

extern "C" int eaqhm_modify_amp_warp(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, double fs,
                                     const double* beta, const double* f_in, const double* f_out, int32_t B,
                                     double* amp) {
  if (!ctx) return EAQHM_EINVAL;
  if (!records || !beta || !f_in || !f_out || !amp || No_ti < 4 || Kmax <= 0 || !finite_pos(fs))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_amp_warp: bad argument");
  if (B < 1 || B > WARP_BMAX) return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_amp_warp: need 1 <= B <= 16 breakpoints");
  const size_t lds = warp_lds_bytes(Kmax);
  if (lds > ENVELOPE_LDS_MAX) return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_amp_warp: Kmax too large for the envelope nodes");
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_modify_amp_warp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  hipLaunchKernelGGL(eaqhm_modify_amp_warp_kernel, dim3((unsigned)((No_ti + PREP_WAVES - 1) / PREP_WAVES)),
                     dim3(64 * PREP_WAVES), lds, ctx->stream, records, (int)No_ti, (int)Kmax, fs, beta, f_in, f_out,
                     (int)B, amp);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_model_envelope_warp(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax,
                                         const double* f_in, const double* f_out, int32_t B, const double* freqs,
                                         int32_t F, double* out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!records || !f_in || !f_out || !freqs || !out || No_ti < 4 || Kmax <= 0 || F <= 0)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_model_envelope_warp: bad argument");
  if (B < 1 || B > WARP_BMAX) return ctx->fail(EAQHM_EINVAL, "eaqhm_model_envelope_warp: need 1 <= B <= 16 breakpoints");
  const size_t lds = warp_lds_bytes(Kmax);
  if (lds > ENVELOPE_LDS_MAX)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_model_envelope_warp: Kmax too large for the envelope nodes");
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_model_envelope_warp_kernel,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(eaqhm_model_envelope_warp_kernel, dim3((unsigned)((No_ti + PREP_WAVES - 1) / PREP_WAVES)),
                     dim3(64 * PREP_WAVES), lds, ctx->stream, records, (int)No_ti, (int)Kmax, f_in, f_out, (int)B, freqs,
                     (int)F, out);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
