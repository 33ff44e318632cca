// eaqhm_modify.hip — resynthesis from an eaQHM model with a time scale rho and a pitch scale beta.
// gfx950 (MI355X) only, FP64.  The definition is in DESIGN.md ("Resynthesis from the model"); at rho = beta = 1 it
// reproduces eaqhm_eval_kernel's synthesis (functions.py:337-385, :537-575) of the same records.
//
//   eaqhm_modify_prep_kernel   one wave per instant: the pitch-scaled knot amplitudes A' (log-amplitude envelope of
//                              the instant's active slots, sorted in LDS, one binary search per slot) and the
//                              unwrapped phase increment Delta of every in-run interval that starts at the instant.
//   eaqhm_modify_scan_kernel   segmented prefix sum of Delta along the instants of each slot (chunks of SCAN_CH
//                              instants: pass 0 chunk aggregates, pass 1 applies the carries), giving the unwrapped
//                              knot phase R and the phase of each run's first knot.
//   eaqhm_modify_carry_kernel  one wave per slot: exclusive segmented scan of the chunk aggregates (the carries).
//   eaqhm_modify_eval_kernel   blocks of output samples: the touched intervals are integrated once into LDS (as
//                              stage 1 of eaqhm_eval_kernel), then per (sample, slot) A * cos(phase), per sample the
//                              a0 spline and the sum over slots in slot order.
#include "eaqhm_common.h"
#include "eaqhm_pieces.h"

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

// ------------------------------------------------------------------------------------------------
// Prep: one wave per instant i (four per block).
//   A'[i][k]  beta == 1: am.  Otherwise, with the envelope, exp(E_i(beta f)) where E_i interpolates ln am linearly over
//             the instant's active slots sorted by (f, k) (flat outside, the first of tied nodes at a node's own
//             frequency), without it am; both muted where beta f >= fs/2.
//   dR[i+1][k] Delta of the interval (i, i+1) when it is in a run: (ph_{i+1} - ph_i) + 2 pi Mr.  Other rows 0.
//   P0[i][k]  ph_i at the first knot of a run (code != 0, previous instant inactive), else 0.
#define PREP_WAVES 4
extern "C" __global__ void __launch_bounds__(64 * PREP_WAVES)
    eaqhm_modify_prep_kernel(ModArgs A, double beta, int envelope, double* __restrict__ amp, double* __restrict__ dR,
                             double* __restrict__ P0) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int K = A.Kmax, D = A.step, RS = 3 * K + 1;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * PREP_WAVES + w;
  double* nf = lds + (size_t)w * 2 * K;   // sorted node frequencies [K] and log amplitudes [K] of this wave's instant
  double* nv = nf + K;
  const bool live = i < A.No_ti;
  const double* row = A.records + (size_t)(live ? i : 0) * RS;
  const bool env = live && beta != 1.0 && envelope;
  int nn = 0;
  if (env) {
    // rank of every active slot in (f, k) order: slots are nearly sorted already, K is at most a few hundred
    for (int k = lane; k < K; k += 64) {
      const double ak = row[k], fk = row[K + k];
      if (ak != 0.0 && fk > 0.0) {
        int rank = 0;
        for (int q = 0; q < K; ++q) {
          const double aq = row[q], fq = row[K + q];
          rank += (aq != 0.0 && fq > 0.0 && (fq < fk || (fq == fk && q < k))) ? 1 : 0;
        }
        nf[rank] = fk;
        nv[rank] = log(ak);
      }
    }
    for (int k = lane; k < K; k += 64) nn += (row[k] != 0.0 && row[K + k] > 0.0) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) nn += __shfl_xor(nn, o);
  }
  __syncthreads();
  if (!live) return;
  const double scale = 2.0 * M_PI / A.fs;
  for (int k = lane; k < K; k += 64) {
    // ---- A'
    const double ak = row[k], fk = row[K + k];
    double a = ak;
    if (beta != 1.0) {
      a = 0.0;
      if (ak != 0.0 && fk > 0.0) {
        const double q = beta * fk;
        a = ak;
        if (envelope) {
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
          a = exp(E);
        }
        if (q >= 0.5 * A.fs) a = 0.0;
      }
    }
    amp[(size_t)i * K + k] = a;
    // ---- Delta of the interval (i, i+1), first-knot phase
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
      }
      dR[(size_t)(i + 1) * K + k] = d;
    }
  }
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

// Block of TBS consecutive output samples x all slots.
//   stage 0  per sample: interval j and offset r (LDS).
//   stage 1  one thread per (interval, slot) touching the block: the interval's local phase
//            Psi(u) = R_j + sum_{v=1..u} w(v) - sum_{v=0..u} sin(pi v/D) er, u = 0..D, in the eval kernel's summation
//            order; at each of the block's samples in the interval the phase P0 + beta rho ((1-fr) Psi(u0) + fr Psi(u0+1))
//            goes to X[k][s].  A run's last knot (tau = c_b) is the end u = D of its last interval.
//   stage 2  one thread per (sample, slot group): amplitude, A cos(phase), isolated knots; then one thread per sample
//            adds the slots in slot order and the a0 spline.
extern "C" __global__ void __launch_bounds__(256) eaqhm_modify_eval_kernel(MEvalArgs E, int TBS, int NR) {
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
  const int tid = threadIdx.x;
  const long long t0 = E.t_lo + (long long)blockIdx.x * TBS;
  const long long t1 = (t0 + TBS < E.t_hi) ? (t0 + TBS) : E.t_hi;
  const int ns = (int)(t1 - t0);
  int jfirst, jlast;
  double rdummy;
  locate(t0, E.rho, D, jfirst, rdummy);
  locate(t1 - 1, E.rho, D, jlast, rdummy);
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
  }
  for (int u = tid; u <= D; u += blockDim.x) ft[u] = sin(M_PI * (double)u / (double)D);
  for (int s = tid; s < ns; s += blockDim.x) {
    int j; double r;
    locate(t0 + s, E.rho, D, j, r);
    sj[s] = j; sr[s] = r;
  }
  __syncthreads();
  const double br = E.beta * E.rho;
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
      acc = w0;
      double c = ft[0] * er;
      double prev = Rj + ((acc - w0) - c);
      int q = sa;
      // u = 0: samples on the knot itself
      while (q < sb && sr[q] == 0.0) { X[(size_t)k * TP + q] = ph0 + br * prev; ++q; }
      for (int u = 1; u <= D; ++u) {
        acc += scale * P(u);
        c += ft[u] * er;
        const double psi = Rj + ((acc - w0) - c);
        while (q < sb) {
          const double rq = sr[q], u0 = floor(rq), fr = rq - u0;
          if ((int)u0 == u - 1 && fr > 0.0) X[(size_t)k * TP + q] = ph0 + br * ((1.0 - fr) * prev + fr * psi);
          else if ((int)u0 == u && fr == 0.0) X[(size_t)k * TP + q] = ph0 + br * psi;
          else break;
          ++q;
        }
        prev = psi;
      }
      if (sl >= 0) X[(size_t)k * TP + sl] = ph0 + br * prev;
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
    const double tau = (double)n / E.rho;
    const double hw = 0.5 / E.rho + 1.0;
    const int ilo = max(0, (int)floor((tau - hw) / (double)D)), ihi = min(A.No_ti - 1, (int)floor((tau + hw) / (double)D) + 1);
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
      for (int i = ilo; i <= ihi; ++i) {   // isolated accepted knots land on the output sample nearest to rho c_i
        if (Sl.code(i) == 1 && (long long)rint(E.rho * ((double)i * (double)D)) == n)
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
    const double tau = (double)n / E.rho;
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

extern "C" int eaqhm_modify_prep(eaqhm_ctx* ctx, const double* records, const uint8_t* code, const double* mom,
                                 int32_t No_ti, int32_t Kmax, int32_t step, double fs, double beta,
                                 int32_t preserve_envelope, double* amp, double* R, double* ph0) {
  if (!ctx) return EAQHM_EINVAL;
  if (!records || !code || !mom || !amp || !R || !ph0 || No_ti < 4 || Kmax <= 0 || step <= 0 || !finite_pos(fs))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_prep: bad argument");
  if (!finite_pos(beta)) return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_prep: beta must be finite and > 0");
  const ModArgs A{records, code, mom, No_ti, Kmax, step, fs};
  const size_t lds = (size_t)PREP_WAVES * 2 * Kmax * sizeof(double);
  if (lds > 64 * 1024) return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_prep: Kmax too large for the envelope nodes");
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_modify_prep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(eaqhm_modify_prep_kernel, dim3((unsigned)((No_ti + PREP_WAVES - 1) / PREP_WAVES)), dim3(64 * PREP_WAVES),
                     lds, ctx->stream, A, beta, (int)(preserve_envelope != 0), amp, R, ph0);
  HIP_TRY(ctx, hipGetLastError());
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
// rows follow the block's tau-span (TBS / rho samples), capped by the LDS budget (rows beyond it are read from memory)
static size_t modify_lds_bytes(int K, int step, int tbs, int nr) {
  return (((size_t)step + 2) & ~(size_t)1) * 8 + (size_t)K * (tbs + 1) * 8 + (size_t)tbs * 8 +
         (size_t)nr * ((3 * (size_t)K + 1) + (K + 1)) * 8 + (((size_t)tbs + 1) & ~(size_t)1) * 4 +
         (((size_t)nr * K + 7) & ~(size_t)7);
}

static int modify_block_samples(int Kmax, int step, double rho, size_t* lds_bytes, int* nr) {
  for (int tbs = 64; tbs >= 16; tbs >>= 1) {
    int NR = (int)ceil((double)(tbs - 1) / (rho * (double)step)) + 6;
    while (NR > 4 && modify_lds_bytes(Kmax, step, tbs, NR) > 78 * 1024) --NR;
    const size_t bytes = modify_lds_bytes(Kmax, step, tbs, NR);
    if (bytes <= 78 * 1024 || tbs == 16) {
      *lds_bytes = bytes; *nr = NR;
      return tbs;
    }
  }
  return 16;
}

extern "C" int eaqhm_modify_synth(eaqhm_ctx* ctx, const double* records, const uint8_t* code, const double* mom,
                                  const double* amp, const double* R, const double* ph0, int32_t No_ti, int32_t Kmax,
                                  int32_t step, double fs, double rho, double beta, int64_t L_out, int64_t t_lo,
                                  int64_t t_hi, double* out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!records || !code || !mom || !amp || !R || !ph0 || !out || No_ti < 4 || Kmax <= 0 || step <= 0 || !finite_pos(fs))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_synth: bad argument");
  if (!finite_pos(rho) || !finite_pos(beta))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_synth: rho and beta must be finite and > 0");
  if (L_out <= 0 || t_lo < 0 || t_hi > L_out || t_lo >= t_hi)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_synth: [t_lo, t_hi) outside [0, L_out)");
  size_t lds_bytes = 0;
  int NR = 0;
  const int TBS = modify_block_samples(Kmax, step, rho, &lds_bytes, &NR);
  if (lds_bytes > 160 * 1024) return ctx->fail(EAQHM_EINVAL, "eaqhm_modify_synth: Kmax too large for the LDS tables");
  const MEvalArgs E{ModArgs{records, code, mom, No_ti, Kmax, step, fs}, amp, R, ph0, rho, beta, (long long)t_lo,
                    (long long)t_hi, out};
  const long long nblocks = (t_hi - t_lo + TBS - 1) / TBS;
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_modify_eval_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds_bytes));
  hipLaunchKernelGGL(eaqhm_modify_eval_kernel, dim3((unsigned)nblocks), dim3(256), lds_bytes, ctx->stream, E, TBS, NR);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
