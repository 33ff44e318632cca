// eaqhm_interp.hip — track interpolation, phase integration, additive synthesis and SRER.
// gfx950 (MI355X) only, FP64.
//
//   eaqhm_spline_kernel   one block per tile of 32 instants x 16 slots, its rows of the records (41 instants of halo
//                         either side) staged in LDS once: runs of consecutive accepted instants
//                         (functions.py:350-362) and the not-a-knot cubic second derivatives on their knots
//                         (functions.py:340, :367; interp1d(kind=3)) through the closed-form inverse of the
//                         (1,4,1) system — a local 69-term sum instead of a sequential tridiagonal sweep.
//   eaqhm_spline_edge_kernel  not-a-knot end conditions of every run from its neighbours' moments.
//   eaqhm_eval_kernel     one block per group of whole knot intervals (about 45 samples; 16-64 samples of an
//                         interval where the step is larger) x all slots: each knot interval is integrated once (linear
//                         am, functions.py:364; cubic fm, :367-371 incl. the padded <4-knot case; phase by
//                         frequency integration with the sine-bump correction, :537-575) into LDS tables; then
//                         per (sample, slot) the next-iteration frequency from the unwrapped phase (:375) and
//                         am*cos(ph); per sample the synthesis a0 + 2*sum am*cos(ph) (:385) and the partial sums
//                         of the reconstruction error (:388).  Every (slot, sample) cell of the two dense
//                         outputs is written, so no memset is needed between adaptations.
//   eaqhm_srer_kernel     deterministic final reduction + SRER in dB.
//
// Bandwidth-type stage: per adaptation it reads (1+3*Kmax)*8*No_ti bytes of records and writes
// 2*Kmax*8*L bytes of dense tracks (the reference keeps seven dense L x Kmax arrays; only am_current and
// fm_current are ever read again, so only those two are materialised here).
#include "eaqhm_common.h"
#include "eaqhm_pieces.h"

namespace eaqhm {

// ------------------------------------------------------------------------------------------------
// Not-a-knot cubic spline moments on uniformly spaced knots, one thread per (instant, slot).
//
// For a run of m >= 4 knots the second derivatives satisfy 6*M_1 = d_1, 6*M_{m-2} = d_{m-2},
// M_0 = 2*M_1 - M_2, M_{m-1} = 2*M_{m-2} - M_{m-3}, and for the n = m-4 inner knots the (1,4,1) Toeplitz
// system T x = dt with dt = d (minus M_1 / M_{m-2} in its first / last row).  T^-1 is known in closed form:
//   (T^-1)_{ij} = (-1)^(i+j) lam^(|i-j|+1) (1-lam^(2 min(i,j))) (1-lam^(2 (n+1-max(i,j))))
//                 / ((1-lam^2) (1-lam^(2(n+1)))),         lam = 2 - sqrt(3),
// and lam^35 < 1e-20, so every moment is a 69-term local sum: no sequential sweep over the (possibly tens
// of thousands of) knots of a run, and only the distance to the run's ends up to 40 knots is ever needed.
#define SPL_W 34
#define SPL_CAP 40
#define SPL_BIG 1000000

// A block of eaqhm_spline_kernel solves SPL_TI instants x SPL_TS columns (slots; the a0 spline is column Kmax) from a
// tile of the records in LDS: rows [first instant - SPL_HALO, last instant + SPL_HALO] of the accepted flag (the am
// column; a0 is accepted everywhere) and of the value (the fm column, or a0).  The run masks look SPL_CAP + 1 rows
// either way and the 69-term sum SPL_W + 2, so 41 rows of halo hold every read.
#define SPL_HALO 41
#define SPL_TI 32
#define SPL_TS 16

static_assert(SPL_TI + 2 * SPL_HALO <= 128, "the accepted flags of a tile column are kept as 128 bits");

struct SplineCol {
  const double* ys; int base, kk; double h2;
  __device__ double y(int i) const { return ys[(i - base) * SPL_TS + kk]; }
  __device__ double d2(int i) const { return 6.0 * ((y(i - 1) - 2.0 * y(i)) + y(i + 1)) / h2; }
};

__device__ inline double lam_pow(const double* lp, int e) { return e > 79 ? 0.0 : lp[e]; }

// moment of a knot that is neither the first nor the last of its run; A / B = distance (in knots) to the
// first / last knot of the run (>= 1), SPL_BIG when farther than SPL_CAP
__device__ double inner_moment(const SplineCol& C, const double* lp, const double* wt, int i, int A, int B) {
  if (A == 1 || B == 1) return C.d2(i) / 6.0;
  if (A >= SPL_BIG && B >= SPL_BIG) {
    // farther than SPL_CAP from both ends of the run (most knots of a long run): the general expression below
    // multiplies every weight by 1.0 twice and subtracts nothing from any row, so the weights come from the table
    // wt[ad] = lam^(ad+1) / (1 - lam^2) — the same sum, term by term
    const double ih2 = 6.0 / C.h2;
    double ym = C.y(i - SPL_W - 1), y0 = C.y(i - SPL_W), yp;
    double acc = 0.0;
    for (int d = -SPL_W; d <= SPL_W; ++d) {
      yp = C.y(i + d + 1);
      const double rhs = ((ym - 2.0 * y0) + yp) * ih2;
      const int ad = d < 0 ? -d : d;
      const double w = wt[ad];
      acc += (ad & 1) ? -w * rhs : w * rhs;
      ym = y0; y0 = yp;
    }
    return acc;
  }
  const int dlo = (A >= SPL_BIG) ? -SPL_W : max(-SPL_W, 2 - A);
  const int dhi = (B >= SPL_BIG) ? SPL_W : min(SPL_W, B - 2);
  const double lam2 = lp[2];
  const double np1 = (A >= SPL_BIG || B >= SPL_BIG) ? 0.0 : lam_pow(lp, 2 * (A + B - 2));  // lam^(2(n+1))
  const double iden = 1.0 / ((1.0 - lam2) * (1.0 - np1)), ih2 = 6.0 / C.h2;   // no division inside the 69-term loop
  double ym = C.y(i + dlo - 1), y0 = C.y(i + dlo), yp;
  double acc = 0.0;
  for (int d = dlo; d <= dhi; ++d) {
    yp = C.y(i + d + 1);
    double rhs = ((ym - 2.0 * y0) + yp) * ih2;
    if (A < SPL_BIG && A + d == 2) rhs -= C.d2(i + d - 1) / 6.0;   // first inner row: - M_1
    if (B < SPL_BIG && B - d == 2) rhs -= C.d2(i + d + 1) / 6.0;   // last inner row:  - M_{m-2}
    const int ad = d < 0 ? -d : d;
    // min(i', j') = A-1+min(d,0);  n+1-max(i', j') = B-1-max(d,0)
    const double fa = (A >= SPL_BIG) ? 1.0 : 1.0 - lam_pow(lp, 2 * (A - 1 + (d < 0 ? d : 0)));
    const double fb = (B >= SPL_BIG) ? 1.0 : 1.0 - lam_pow(lp, 2 * (B - 1 - (d > 0 ? d : 0)));
    const double w = (lam_pow(lp, ad + 1) * fa) * (fb * iden);
    acc += (ad & 1) ? -w * rhs : w * rhs;
    ym = y0; y0 = yp;
  }
  return acc;
}

extern "C" __global__ void __launch_bounds__(256) eaqhm_spline_kernel(const double* __restrict__ records, int No_ti,
                                                                      int i0, int ni, int Kmax, int step,
                                                                      unsigned char* __restrict__ code,
                                                                      double* __restrict__ mom) {
  __shared__ double lp[80];
  __shared__ double ys[(SPL_TI + 2 * SPL_HALO) * SPL_TS];
  __shared__ unsigned char as[(SPL_TI + 2 * SPL_HALO) * SPL_TS];
  __shared__ double wt[SPL_W + 1];
  __shared__ unsigned long long cm[SPL_TS][2];   // a column's accepted flags: row r of the tile is bit r
  if (threadIdx.x < 80) lp[threadIdx.x] = pow(2.0 - sqrt(3.0), (double)threadIdx.x);
  const int ld = Kmax + 1, nS = (ld + SPL_TS - 1) / SPL_TS;
  const int ia = i0 + (int)(blockIdx.x / nS) * SPL_TI, ib = min(ia + SPL_TI, i0 + ni);   // instants [ia, ib)
  const int k0 = (int)(blockIdx.x % nS) * SPL_TS;
  const int base = ia - SPL_HALO, nrow = ib - ia + 2 * SPL_HALO;
  {
    // one row of the tile is SPL_TS neighbouring columns of a record: coalesced along the slot axis
    const size_t RS = 3 * (size_t)Kmax + 1;
    for (int q = threadIdx.x; q < nrow * SPL_TS; q += blockDim.x) {
      const int i = base + q / SPL_TS, k = k0 + q % SPL_TS;
      double y = 0.0;
      unsigned char a = 0;
      if (i >= 0 && i < No_ti && k < ld) {
        const double* row = records + (size_t)i * RS;
        if (k == Kmax) { y = row[3 * Kmax]; a = 1; }
        else { y = row[Kmax + k]; a = row[k] != 0.0; }
      }
      ys[q] = y; as[q] = a;
    }
  }
  __syncthreads();
  {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;   // (256 threads: four waves)
    for (int c = w; c < SPL_TS; c += 4) {
      const unsigned long long lo = __ballot(l < nrow && as[l * SPL_TS + c] != 0);
      const unsigned long long hi = __ballot(64 + l < nrow && as[(64 + l) * SPL_TS + c] != 0);
      if (l == 0) { cm[c][0] = lo; cm[c][1] = hi; }
    }
    if (threadIdx.x <= SPL_W) {
      const double lam2 = lp[2], np1 = 0.0;
      const double iden = 1.0 / ((1.0 - lam2) * (1.0 - np1));
      wt[threadIdx.x] = (lp[threadIdx.x + 1] * 1.0) * (1.0 * iden);
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < (ib - ia) * SPL_TS; q += blockDim.x) {
    const int i = ia + q / SPL_TS, kk = q % SPL_TS, k = k0 + kk;
    if (k >= ld) continue;
    SplineCol C;
    C.ys = ys; C.base = base; C.kk = kk;
    C.h2 = (double)step * (double)step;
    double M = 0.0;
    unsigned char cd = 0;
    const int p = i - base;   // the instant's row in the tile: SPL_HALO <= p < SPL_HALO + SPL_TI
    const unsigned long long m0 = cm[kk][0], m1 = cm[kk][1];
    if (((p < 64 ? m0 >> p : m1 >> (p - 64)) & 1ull) != 0) {
      // accepted neighbours on both sides as bit masks (bit d: the instant d + 1 away), then the run lengths are the
      // trailing ones of the masks
      const int sr = p + 1;   // 42 .. 73
      const unsigned long long mr = (sr < 64 ? (m0 >> sr) | (m1 << (64 - sr)) : m1 >> (sr - 64)) & ((1ull << SPL_CAP) - 1);
      // rows p-1, p-2, ... from bit 63 downwards
      const unsigned long long lt = p < 64 ? m0 << (64 - p) : (p == 64 ? m0 : (m1 << (128 - p)) | (m0 >> (p - 64)));
      const int dl = min(SPL_CAP, ~lt ? (int)__clzll((long long)~lt) : 64), dr = min(SPL_CAP, __ffsll((long long)~mr) - 1);
      const bool kl = dl < SPL_CAP, kr = dr < SPL_CAP;
      const int m = dl + dr + 1;
      if (kl && kr && m < 4) {
        cd = (m == 1) ? 1 : (unsigned char)(16 + 4 * m + dl);
      } else {
        cd = 2;
        const int A = kl ? dl : SPL_BIG, B = kr ? dr : SPL_BIG;
        // the first / last knot of a run takes 2 M_1 - M_2 from its neighbours' moments: eaqhm_spline_edge_kernel
        // (computing them here would make every wave that holds one edge knot run the 69-term sum three times)
        if (A != 0 && B != 0) M = inner_moment(C, lp, wt, i, A, B);
      }
    }
    mom[(size_t)i * ld + k] = M;
    if (k < Kmax) code[(size_t)i * Kmax + k] = cd;
  }
}

// not-a-knot end conditions: M_0 = 2 M_1 - M_2 and M_{m-1} = 2 M_{m-2} - M_{m-3} for runs of m >= 4 knots (code 2)
extern "C" __global__ void __launch_bounds__(256) eaqhm_spline_edge_kernel(const unsigned char* __restrict__ code, int No_ti,
                                                                           int i0, int ni, int Kmax, double* __restrict__ mom) {
  const int ld = Kmax + 1;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)ni * ld) return;
  const int i = i0 + (int)(idx / ld), k = (int)(idx % ld);
  auto acc = [&](int q) { return q >= 0 && q < No_ti && (k == Kmax || code[(size_t)q * Kmax + k] != 0); };
  if (!(k == Kmax || code[(size_t)i * Kmax + k] == 2)) return;
  const bool first = !acc(i - 1), last = !acc(i + 1);
  if (first == last) return;   // inner knot (or isolated: not code 2)
  const int s1 = first ? 1 : -1;
  mom[(size_t)i * ld + k] = 2.0 * mom[(size_t)(i + s1) * ld + k] - mom[(size_t)(i + 2 * s1) * ld + k];
}

// ------------------------------------------------------------------------------------------------
struct EvalArgs {
  const double* records; const unsigned char* code; const double* mom;
  int No_ti; int Kmax; int step; double fs; long long L; long long t_lo; long long t_hi; long long s_lo; long long s_hi;
  int eshift;   // error_sum_shift(std_det)
  // am_out / fm_out: biased by -track_t0, rows of Lt samples (only samples [t_lo, t_hi) are written); NULL: no track
  // output.  s_hat NULL: no synthesis, no phase rows, no error sums (a pass that only regenerates tracks).
  const double* target; double* am_out; double* fm_out; long long Lt; double* ph_knot; double* s_hat; long long* partials;
};

// ---- error sums that do not depend on how the samples are grouped -------------------------------------------------
// SRER (functions.py:388) needs sum d and sum d^2 over the whole file, d = target - s_hat.  They are collected per
// block, per rank and (long files) per time block; a floating-point sum would make the last digits of the SRER — and
// with them the stop rule `SRER[a] <= SRER[a-1]` — depend on that grouping.  So every sample is turned into fixed
// point and the limbs are added as integers: exact, associative, identical for every block size, world size and
// streaming block.  The resolution follows the signal: with std_det = m * 2^e, 0.5 <= m < 1 (frexp), the shift is
// s = 10 - e (0 for a std_det that is zero or not finite, clamped to +-ES_SHIFT_MAX), which puts std_det * 2^s into
// [2^9, 2^10), and d' = d * 2^s (exact) is what is summed: rint(d' * 2^60) and rint(d'^2 * 2^64), to nearest, ties to
// even, three signed 64-bit limbs in base 2^32 each.  |d'| < 2^30 is required (anything larger — an error a million
// times the signal's own level — and NaN / Inf is counted in limb 6 and reported by the host); the squared error is
// resolved to 2^-84 of the squared level, which keeps the SRER to 1e-7 dB up to 180 dB.  The top limb of one sample
// stays below 2^60; what bounds the int64 sums is the sum itself, sum d'^2 < 2^63 (include/eaqhm_hip.h).  The shift travels in limb 7:
// the words say at which scale they were taken, and s = 0 is the plain d * 2^60, d^2 * 2^64.
#define ES_LIMBS 8   // {d': l0, l1, l2,  d'^2: l0, l1, l2,  non-finite or huge samples, the shift s}
#define ES_SHIFT_MAX 900
__host__ __device__ inline int error_sum_shift(double std_det) {
  if (!(std_det > 0.0) || std_det > 1.7e308) return 0;
  int e;
  frexp(std_det, &e);
  const int s = 10 - e;
  return s > ES_SHIFT_MAX ? ES_SHIFT_MAX : (s < -ES_SHIFT_MAX ? -ES_SHIFT_MAX : s);
}
__device__ inline void fixed_limbs(double x, long long& l0, long long& l1, long long& l2) {
  // x already scaled by a power of two (exact); |x| < 2^126
  x = rint(x);                                // to nearest; from here on every step is exact
  const double h2 = trunc(x * 0x1p-64);
  const double r1 = x - h2 * 0x1p64;          // exact: the low bits of x
  const double h1 = trunc(r1 * 0x1p-32);
  const double r0 = r1 - h1 * 0x1p32;         // exact
  l2 = (long long)h2; l1 = (long long)h1; l0 = (long long)r0;
}

// Rows [r0, r1] of records / code / mom staged in LDS by the block (eaqhm_eval_kernel); anything outside (only the
// padded <4-knot case reaches back to rows 0..3) is read from memory.
struct RowCache {
  const double* rec; const double* mom; const unsigned char* code; int r0, r1;
};

struct Slot {
  const EvalArgs& A;
  const RowCache& C;
  int k;
  __device__ bool in(int i) const { return i >= C.r0 && i <= C.r1; }
  __device__ double recv(int i, int col) const {
    const int RS = 3 * A.Kmax + 1;
    return in(i) ? C.rec[(size_t)(i - C.r0) * RS + col] : A.records[(size_t)i * RS + col];
  }
  __device__ double am(int i) const { return recv(i, k); }
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

// numpy.unwrap on one step: the unwrapped difference
__device__ inline double unwrap_diff(double dd) {
  if (fabs(dd) < M_PI) return dd;
  double m = fmod(dd + M_PI, 2.0 * M_PI);
  if (m < 0) m += 2.0 * M_PI;
  m -= M_PI;
  if (m == -M_PI && dd > 0) m = M_PI;
  return m;
}

// Block of up to TBS consecutive samples x all slots.  Blocks sit on a grid that is fixed to sample 0 whatever the
// range: block B owns the samples (B*TBS - TBS, B*TBS], clipped to [t_lo, t_hi) (block 0 is sample 0 alone).  Where the
// step allows, TBS is a multiple of it, so a block owns whole knot intervals and every interval is integrated by
// exactly one block; a step larger than a block leaves blocks that cover part of an interval.
//   stage 1  one thread per (knot interval, slot) touching the block: phase_integr_interpolation
//            (functions.py:537-575) of the whole interval ONCE, in the reference's summation order — cumulative
//            sum of the instantaneous frequency, shifted to start at the analysed phase, minus the cumulative
//            sine bump that closes the phase error at the next knot.  The running sum goes to LDS as it is formed and
//            takes the shift and the bump in place once the closing error is known, so the piece is evaluated once per
//            sample.  X1[k][c] phase at sample t0 + c (c = 0: the sample before the block's first), XS[k][interval]
//            phase at the interval's first sample as the interval itself integrates it, XA[k][interval] the slope of
//            the linear amplitude, X3[k][knot] fm_recon at the
//            first sample of the interval that starts at the knot (for the block's last knot that interval belongs
//            to the next block: only its P(0) is taken).
//   stage 2  one thread per (sample, slot group): amplitudes, next-iteration frequency from the unwrapped phase
//            (functions.py:375; "one sample earlier" is the neighbouring cell of X1, or XS at an interval's first
//            sample), knot bookkeeping, am*cos(ph) into LDS; then one thread per sample adds the slots in slot order,
//            the a0 spline and the reconstruction error (functions.py:385-388).
extern "C" __global__ void __launch_bounds__(256) eaqhm_eval_kernel(EvalArgs A, int TBS, int NK, int NI, int NR,
                                                                    long long B0) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int D = A.step, K = A.Kmax;
  double* ft = lds;                           // D+1
  double* X1 = lds + ((D + 1 + 1) & ~1);      // [K][TP]
  const int TP = (TBS + 1) | 1;               // odd row stride: stage 1 writes a column of slots at once (bank spread)
  double* X3 = X1 + (size_t)K * TP;           // [K][NK]
  double* XS = X3 + (size_t)K * NK;           // [K][NI]
  double* XA = XS + (size_t)K * NI;           // [K][NI]
  double* crec = XA + (size_t)K * NI;         // [NR][3K+1]   staged rows of the records
  double* cmom = crec + (size_t)NR * (3 * K + 1);                    // [NR][K+1]
  unsigned char* ccode = (unsigned char*)(cmom + (size_t)NR * (K + 1));   // [NR][K]
  const int tid = threadIdx.x;
  const long long Bi = B0 + blockIdx.x;
  const long long t1 = Bi * TBS, t0 = (Bi == 0) ? -1 : t1 - TBS;      // the block owns (t0, t1] ...
  const long long cl = (t0 + 1 > A.t_lo) ? t0 + 1 : A.t_lo;           // ... of which [cl, ch] lie in the range (never empty)
  const long long ch = (t1 < A.t_hi - 1) ? t1 : A.t_hi - 1;
  const long long tk0 = ((t0 + D) / D) * D;                           // first knot after t0
  // intervals (j, j+1) that hold one of the samples [cl, ch] past their first
  const int jlo = (cl > 0) ? (int)((cl - 1) / D) : 0, jhi = (ch > 0) ? (int)((ch - 1) / D) : -1;
  const int nint = jhi - jlo + 1;
  // the instants this block touches: one before its first interval to two after its last (coalesced rows)
  RowCache C;
  {
    C.r0 = (jlo > 0) ? jlo - 1 : 0;
    C.r1 = (jhi + 2 < A.No_ti) ? jhi + 2 : A.No_ti - 1;
    if (C.r1 > C.r0 + NR - 1) C.r1 = C.r0 + NR - 1;
    if (C.r1 < C.r0) C.r1 = C.r0 - 1;   // nothing staged (block beyond the last instant)
    C.rec = crec; C.mom = cmom; C.code = ccode;
    const int nrow = C.r1 - C.r0 + 1, RS = 3 * K + 1;
    for (int q = tid; q < nrow * RS; q += blockDim.x) crec[q] = A.records[(size_t)C.r0 * RS + q];
    for (int q = tid; q < nrow * (K + 1); q += blockDim.x) cmom[q] = A.mom[(size_t)C.r0 * (K + 1) + q];
    for (int q = tid; q < nrow * K; q += blockDim.x) ccode[q] = A.code[(size_t)C.r0 * K + q];
  }
  for (int u = tid; u <= D; u += blockDim.x) ft[u] = sin(M_PI * (double)u / (double)D);
  __syncthreads();
  // ---- stage 1: the intervals jlo .. jhi, and P(0) of interval jhi + 1 where it starts on a sample of the block
  {
    const double scale = 2.0 * M_PI / A.fs;
    for (int p = tid; p < (nint + 1) * K; p += blockDim.x) {
      const int jj = p / K, k = p - jj * K, j = jlo + jj;
      if (j + 1 >= A.No_ti) continue;
      const long long tb = (long long)j * D;
      if (jj == nint && tb > ch) continue;
      Slot S{A, C, k};
      const int cj = S.code(j);
      if (cj == 0 || S.code(j + 1) == 0) continue;
      const FmPiece P = make_piece(S, j, cj);
      const double p0 = P(0), w0 = scale * p0;
      if (tb >= cl && tb <= ch) X3[(size_t)k * NK + (int)((tb - tk0) / D)] = p0;
      if (jj == nint) continue;
      {   // slope of the linear amplitude (functions.py:364), the same for every sample of the interval
        const double x0 = (double)j * (double)D, x1 = (double)(j + 1) * (double)D;
        XA[(size_t)k * NI + jj] = (S.am(j + 1) - S.am(j)) / (x1 - x0);
      }
      // the interval's samples tb + u with ua <= u <= ub have a cell in X1
      const int ua = (int)(t0 - tb), ub = (int)(t1 - tb);
      double* x = X1 + (size_t)k * TP - ua;
      double acc = w0;
      for (int u = 1; u <= D; ++u) {
        acc += scale * P(u);
        if (u >= ua && u <= ub) x[u] = acc;
      }
      const double shift = S.ph(j) - w0;
      const double e = (acc + shift) - S.ph(j + 1);
      const double Mr = rint(e / (2.0 * M_PI));
      const double er = M_PI * (e - 2.0 * M_PI * Mr) / (2.0 * (double)D);
      acc = w0;
      double c = ft[0] * er;
      XS[(size_t)k * NI + jj] = (acc + shift) - c;
      for (int u = 1; u <= D; ++u) {
        c += ft[u] * er;
        if (u >= ua && u <= ub) x[u] = (x[u] + shift) - c;
      }
    }
  }
  __syncthreads();
  // ---- stage 2
  const int s = tid % TBS, g = tid / TBS, G = blockDim.x / TBS;
  const long long t = t0 + 1 + s;
  const bool live = g < G && t >= cl && t <= ch;
  int i = 0, r = 0;
  bool past = false;
  if (live) {
    i = (int)(t / D);
    r = (int)(t - (long long)i * D);
    if (i >= A.No_ti) { i = A.No_ti - 1; r = (int)(t - (long long)i * D); }  // beyond the last instant
    past = (i == A.No_ti - 1) && (r > 0);
  }
  // a thread reads its own cell of X1 and its left neighbour's, and then puts am*cos(ph) into its own: all the reads
  // of a row come before the barrier, and each round of the loop works on rows of its own
  for (int k = g; k - g < K; k += G) {   // (the same number of rounds for every thread: the barrier)
    const bool on = live && k < K;
    double prod = 0.0;
    if (on) {
      Slot S{A, C, k};
      const double* x = X1 + (size_t)k * TP + s + 1;   // this sample's cell
      double amv = 0.0, phv = 0.0, fnext = 0.0;
      const int ci = S.code(i);
      if (!past && r > 0) {
        const int cn = S.code(i + 1);
        if (ci != 0 && cn != 0) {  // inside the active interval (i, i+1)
          const double x0 = (double)i * (double)D;
          amv = XA[(size_t)k * NI + (i - jlo)] * ((double)t - x0) + S.am(i);
          const double pr = x[0], pm = (r == 1) ? XS[(size_t)k * NI + (i - jlo)] : x[-1];
          phv = pr;
          fnext = A.fs / (2.0 * M_PI) * unwrap_diff(pr - pm);
        }
      } else if (r == 0) {
        if (ci != 0) {  // on a knot
          amv = S.am(i);
          const bool prev = S.code(i - 1) != 0, next = S.code(i + 1) != 0;
          if (!prev && !next) {
            phv = S.ph(i);  // isolated accepted instant: frame-centre values stay as written
          } else {
            double pD = 0.0, pDm1 = 0.0;
            if (prev) { pD = x[0]; pDm1 = (D == 1) ? XS[(size_t)k * NI + (i - 1 - jlo)] : x[-1]; }
            if (next) {
              const double p0 = X3[(size_t)k * NK + (int)((t - tk0) / D)];
              const double w0 = (2.0 * M_PI / A.fs) * p0;
              phv = w0 + (S.ph(i) - w0);  // first sample of the next interval overwrites the knot
              if (!prev) fnext = p0;      // first sample of the run keeps fm_recon (functions.py:375)
            } else {
              phv = pD;                   // last knot of a run keeps the integrated phase
            }
            if (prev) fnext = A.fs / (2.0 * M_PI) * unwrap_diff(phv - pDm1);
          }
          if (A.s_hat) A.ph_knot[(size_t)i * K + k] = phv;
        } else {
          if (A.s_hat) A.ph_knot[(size_t)i * K + k] = 0.0;
        }
      }
      if (A.am_out) {
        A.am_out[(size_t)k * A.Lt + t] = amv;
        A.fm_out[(size_t)k * A.Lt + t] = fnext;
      }
      prod = (amv != 0.0) ? amv * cos(phv) : 0.0;
    }
    if (A.s_hat) {   // (uniform over the grid)
      __syncthreads();
      if (on) X1[(size_t)k * TP + s + 1] = prod;
    }
  }
  if (!A.s_hat) return;   // (uniform over the grid: a track-only pass)
  __syncthreads();
  long long e[ES_LIMBS - 1] = {0, 0, 0, 0, 0, 0, 0};
  if (g == 0 && live) {
    double synth = 0.0;
#pragma unroll 8
    for (int k = 0; k < K; ++k) synth += X1[(size_t)k * TP + s + 1];   // slot order; the loads of eight slots in flight
    // a0: not-a-knot spline through every instant, extrapolated past the last one (functions.py:340)
    int ia = i;
    if (ia > A.No_ti - 2) ia = A.No_ti - 2;
    const size_t RS = 3 * (size_t)K + 1;
    Slot S0{A, C, K};   // column K of mom = the a0 spline; its knots are the last record column
    double a0v = spline_piece(S0.recv(ia, (int)RS - 1), S0.recv(ia + 1, (int)RS - 1), S0.mom(ia), S0.mom(ia + 1),
                              (double)(t - (long long)ia * D), (double)D);
    const double sh = a0v + 2.0 * synth;
    A.s_hat[t] = sh;
    if (t >= A.s_lo && t < A.s_hi) {
      const double d = scalbn(A.target[t] - sh, A.eshift);
      if (fabs(d) < 0x1p30) {   // (false for NaN)
        fixed_limbs(d * 0x1p60, e[0], e[1], e[2]);
        fixed_limbs((d * d) * 0x1p64, e[3], e[4], e[5]);
      } else {
        e[6] = 1;
      }
    }
  }
  if (tid < 64) {   // TBS <= 64 (EVAL_SAMPLES_MAX): the block's samples sit in the first wave
#pragma unroll
    for (int q = 0; q < ES_LIMBS - 1; ++q) {
      for (int o = 32; o > 0; o >>= 1) e[q] += __shfl_xor(e[q], o);
      if (tid == 0) A.partials[(size_t)q * gridDim.x + blockIdx.x] = e[q];   // [limb][block]: the reduction reads coalesced
    }
  }
}

// Adds the blocks' limbs (integers: any order gives the same result), carries them into two 128-bit totals and leaves
//   sums_out[0..3]  sum d, sum d^2, n, SRER in dB — doubles, a convenience for C callers; the Python host derives the
//                   SRER itself from the limbs (one formula for every world size and block count)
//   sums_out[4..6]  LS breakdowns / stalled diagonal pipelines / dropped frames since the last read (counters are cleared)
//   sums_out[8..15] the limbs as int64 bit patterns: what ranks and time blocks add up (the last one is the shift, the
//                   same on every rank: it is not added)
extern "C" __global__ void __launch_bounds__(1024) eaqhm_srer_kernel(const long long* partials, long long nblocks, double n,
                                                                    double std_det, double* sums_out, int* faults) {
  __shared__ long long red[16][ES_LIMBS];
  long long e[ES_LIMBS - 1] = {0, 0, 0, 0, 0, 0, 0};
  for (long long b = threadIdx.x; b < nblocks; b += blockDim.x)
#pragma unroll
    for (int q = 0; q < ES_LIMBS - 1; ++q) e[q] += partials[(size_t)q * nblocks + b];
#pragma unroll
  for (int q = 0; q < ES_LIMBS - 1; ++q) {
    for (int o = 32; o > 0; o >>= 1) e[q] += __shfl_xor(e[q], o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = e[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long* lim = (long long*)(sums_out + 8);
    for (int q = 0; q < ES_LIMBS - 1; ++q) {
      e[q] = 0;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) e[q] += red[w][q];
      lim[q] = e[q];
    }
    const int sh = error_sum_shift(std_det);
    lim[ES_LIMBS - 1] = sh;
    // the sums of d' and d'^2; the SRER is a ratio, so it is taken in the scaled domain (std_det * 2^s is in [2^9, 2^10))
    const double a = ((double)e[2] * 0x1p64 + (double)e[1] * 0x1p32 + (double)e[0]) * 0x1p-60;
    const double b = ((double)e[5] * 0x1p64 + (double)e[4] * 0x1p32 + (double)e[3]) * 0x1p-64;
    const double mean = a / n;
    const double var = b / n - mean * mean;
    sums_out[0] = scalbn(a, -sh); sums_out[1] = scalbn(scalbn(b, -sh), -sh); sums_out[2] = n;
    sums_out[3] = e[6] ? __builtin_nan("") : 20.0 * log10(scalbn(std_det, sh) / sqrt(var));
    sums_out[4] = (double)faults[0];   // LS systems whose factorisation broke down in this adaptation (eaqhm_ls_faults)
    sums_out[5] = (double)faults[1];   // diagonal pipelines that timed out (a bug of the library if ever nonzero)
    sums_out[6] = (double)faults[2];   // frames dropped because their window lay outside the resident track window
    faults[0] = 0; faults[1] = 0; faults[2] = 0;
  }
}


// ------------------------------------------------------------------------------------------------
// The third inner seam as a stand-alone entry: phase_integr_interpolation(fm_recon, ph_recon, indices)
// (functions.py:537-575) for arbitrary knot spacing.  One thread per sample of [knots[0], knots[m-1]]; the
// sample's interval is found by binary search; each interval is integrated in the reference's summation
// order (cumulative sum of the instantaneous frequency, shifted to start at the analysed phase, minus the
// cumulative sine bump that closes the phase error at the next knot).  The shared knot of two intervals takes
// the value of the LATER interval (its first sample), the very last knot keeps the integrated value.
extern "C" __global__ void eaqhm_phase_integrate_kernel(const double* __restrict__ omega, const double* __restrict__ ph,
                                                        const int* __restrict__ knots, int m, double* __restrict__ out) {
  const int first = knots[0], last = knots[m - 1];
  const int t = first + blockIdx.x * blockDim.x + threadIdx.x;
  if (t > last) return;
  int lo = 0, hi = m - 1;  // interval i with knots[i] <= t < knots[i+1]  (t == last -> i = m-2)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (knots[mid] <= t) lo = mid; else hi = mid;
  }
  const int i0 = knots[lo], i1 = knots[lo + 1], D = i1 - i0, r = t - i0;
  double acc = omega[i0], sr = acc;
  for (int u = 1; u <= D; ++u) {
    acc += omega[i0 + u];
    if (u == r) sr = acc;
  }
  const double shift = ph[i0] - omega[i0];
  const double e = (acc + shift) - ph[i1];
  const double Mr = rint(e / (2.0 * M_PI));
  const double er = M_PI * (e - 2.0 * M_PI * Mr) / (2.0 * (double)D);
  double c = 0.0, cr = 0.0;
  for (int u = 0; u <= D; ++u) {
    c += sin(M_PI * (double)u / (double)D) * er;
    if (u == r) cr = c;
  }
  out[t - first] = (sr + shift) - cr;
}
}  // namespace eaqhm

using namespace eaqhm;

extern "C" int eaqhm_spline_solve_range(eaqhm_ctx* ctx, const double* records, int32_t No_ti, int32_t Kmax, int32_t step,
                                        int32_t i_lo, int32_t i_hi, uint8_t* code, double* mom) {
  if (!ctx) return EAQHM_EINVAL;
  if (!records || !code || !mom || Kmax <= 0 || step <= 0 || i_lo < 0 || i_hi > No_ti || i_lo >= i_hi)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_spline_solve: bad argument");
  if (No_ti < 4) return ctx->fail(EAQHM_EINVAL, "eaqhm_spline_solve: need at least 4 analysis instants (interp1d kind=3)");
  const int ld = Kmax + 1;
  auto blocks = [&](int n) { return dim3((unsigned)(((long long)n * ld + 255) / 256)); };
  // eaqhm_spline_kernel: tiles of SPL_TI instants x SPL_TS columns
  auto tiles = [&](int n) { return dim3((unsigned)(((n + SPL_TI - 1) / SPL_TI) * ((ld + SPL_TS - 1) / SPL_TS))); };
  // moments two instants beyond the range feed the end conditions of runs that start / stop inside it
  const int a = (i_lo - 2 > 0) ? i_lo - 2 : 0, b = (i_hi + 2 < No_ti) ? i_hi + 2 : No_ti;
  hipLaunchKernelGGL(eaqhm_spline_kernel, tiles(b - a), dim3(256), 0, ctx->stream, records, No_ti, a, b - a, Kmax, step,
                     code, mom);
  HIP_TRY(ctx, hipGetLastError());
  if (a > 0) {   // the padded <4-knot case looks at the run codes of instants 0..3 wherever it is evaluated
    const int n0 = (a < 4) ? a : 4;
    hipLaunchKernelGGL(eaqhm_spline_kernel, tiles(n0), dim3(256), 0, ctx->stream, records, No_ti, 0, n0, Kmax, step, code, mom);
    HIP_TRY(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(eaqhm_spline_edge_kernel, blocks(i_hi - i_lo), dim3(256), 0, ctx->stream, code, No_ti, i_lo,
                     i_hi - i_lo, Kmax, mom);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_spline_solve(eaqhm_ctx* ctx, const double* records, int32_t No_ti,
                                  int32_t Kmax, int32_t step, uint8_t* code, double* mom) {
  return eaqhm_spline_solve_range(ctx, records, No_ti, Kmax, step, 0, No_ti, code, mom);
}

// Launch geometry of eaqhm_eval_kernel.  A step of at most EVAL_SAMPLES: blocks of m whole knot intervals, m the
// largest with m * step <= EVAL_SAMPLES whose LDS tables fit (never fewer than 16 samples: eaqhm_eval_partials_len
// counts on it).  A larger step: the largest of 64/32/16 samples whose tables fit, as parts of an interval.  Either
// way a block holds at most EVAL_SAMPLES_MAX samples: the kernel's error sums are reduced within its first wave.
// 45: measured on synth16k_60s against 30, 60 and 120.
constexpr int EVAL_SAMPLES = 45, EVAL_SAMPLES_MAX = 64;
static_assert(EVAL_SAMPLES >= 16 && EVAL_SAMPLES <= EVAL_SAMPLES_MAX, "blocks of 16 .. 64 samples");
struct EvalGeometry { int TBS, NK, NI, NR; size_t lds_bytes; };
static EvalGeometry eval_geometry(int Kmax, int step) {
  auto make = [&](int tbs, int ni) {
    EvalGeometry g;
    g.TBS = tbs; g.NK = tbs / step + 1; g.NI = ni; g.NR = ni + 3;   // staged instants: one before the intervals, two after
    g.lds_bytes = (((size_t)step + 2) & ~(size_t)1) * 8 +
                  ((size_t)Kmax * ((tbs + 1) | 1) + (size_t)Kmax * g.NK + (size_t)2 * Kmax * g.NI) * 8 +
                  (size_t)g.NR * ((3 * (size_t)Kmax + 1) + (Kmax + 1)) * 8 + (((size_t)g.NR * Kmax + 7) & ~(size_t)7);
    return g;
  };
  const size_t budget = 78 * 1024;   // two blocks per CU at the least
  if (step <= EVAL_SAMPLES) {
    const int m_min = (16 + step - 1) / step;
    int m = EVAL_SAMPLES / step;
    if (m < m_min) m = m_min;
    while (m > m_min && make(m * step, m).lds_bytes > budget) --m;
    return make(m * step, m);
  }
  for (int tbs = 64; tbs > 16; tbs >>= 1) {
    const EvalGeometry g = make(tbs, tbs / step + 2);
    if (g.lds_bytes <= budget) return g;
  }
  return make(16, 16 / step + 2);
}

extern "C" int64_t eaqhm_eval_partials_len(int64_t t_lo, int64_t t_hi, int32_t step) {
  (void)step;
  if (t_hi <= t_lo) return ES_LIMBS;
  // eight 8-byte words per block of >= 16 samples; the blocks sit on a grid fixed to sample 0, so a range touches
  // one block more than its length alone would need
  return ES_LIMBS * ((t_hi - t_lo + 15) / 16 + 1);
}

extern "C" int eaqhm_eval_synth(eaqhm_ctx* ctx, const double* records, const uint8_t* code,
                                const double* mom, int32_t No_ti, int32_t Kmax, int32_t step, double fs, int64_t L,
                                int64_t t_lo, int64_t t_hi, int64_t s_lo, int64_t s_hi, const double* target,
                                double std_det, double* am_out, double* fm_out, int64_t track_t0, int64_t track_len,
                                double* ph_knot, double* s_hat, double* partials, double* sums_out) {
  if (!ctx) return EAQHM_EINVAL;
  const bool tracks = am_out != nullptr, synth = s_hat != nullptr;
  if (!records || !code || !mom || (!tracks && !synth) || (tracks && !fm_out) || No_ti < 4 || Kmax <= 0 || step <= 0 ||
      fs <= 0 || L <= 0 || t_lo < 0 || t_hi > L || t_lo >= t_hi)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_eval_synth: bad argument");
  if (synth && (!target || !ph_knot || !partials || !sums_out || s_lo < t_lo || s_hi > t_hi || s_lo >= s_hi))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_eval_synth: bad argument (synthesis outputs / error range)");
  if (tracks && (track_t0 < 0 || track_len <= 0 || t_lo < track_t0 || t_hi > track_t0 + track_len))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_eval_synth: [t_lo, t_hi) outside the track window");
  if ((int64_t)(No_ti - 1) * step >= L) return ctx->fail(EAQHM_EINVAL, "eaqhm_eval_synth: instants beyond the signal");
  EvalArgs A{records, code, mom, No_ti, Kmax, step, fs, (long long)L, (long long)t_lo, (long long)t_hi,
             (long long)s_lo, (long long)s_hi, error_sum_shift(std_det), target, tracks ? am_out - track_t0 : nullptr,
             tracks ? fm_out - track_t0 : nullptr, (long long)track_len, ph_knot, s_hat, (long long*)partials};
  const EvalGeometry g = eval_geometry(Kmax, step);
  if (g.lds_bytes > 160 * 1024) return ctx->fail(EAQHM_EINVAL, "eaqhm_eval_synth: Kmax too large for the LDS tables");
  // blocks B_lo .. B_hi of the grid fixed to sample 0: block B owns (B*TBS - TBS, B*TBS]
  const long long B_lo = (t_lo + g.TBS - 1) / g.TBS, B_hi = (t_hi - 1 + g.TBS - 1) / g.TBS;
  const long long nblocks = B_hi - B_lo + 1;
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_eval_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds_bytes));
  hipLaunchKernelGGL(eaqhm_eval_kernel, dim3((unsigned)nblocks), dim3(256), g.lds_bytes, ctx->stream, A, g.TBS, g.NK, g.NI,
                     g.NR, B_lo);
  HIP_TRY(ctx, hipGetLastError());
  if (!synth) return EAQHM_OK;
  hipLaunchKernelGGL(eaqhm_srer_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const long long*)partials, nblocks,
                     (double)(s_hi - s_lo), std_det, sums_out, ctx->faults);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_phase_integrate(eaqhm_ctx* ctx, const double* omega, const double* ph, const int32_t* knots,
                                     int32_t n_knots, int32_t first, int32_t last, double* out) {
  if (!ctx) return EAQHM_EINVAL;
  if (!omega || !ph || !knots || !out || n_knots < 2 || last <= first)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_phase_integrate: bad argument");
  const int n = last - first + 1;
  hipLaunchKernelGGL(eaqhm_phase_integrate_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, omega, ph, knots,
                     n_knots, out);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
