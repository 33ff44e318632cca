// eaqhm_formant.hip — formant tracks: the poles of every frame's all-pole envelope, the formant
// candidates among them, and the Viterbi decode that sorts the candidates into F1..FN over time.  gfx950 (MI355X) only.
//
//   eaqhm_allpole_roots_kernel        one wave per frame, four per block.  Lane j holds a_j after the step-up; lane k < pe
//                                     owns the root z_k.  What a step needs from another lane (a_j for the Horner pass,
//                                     z_j for the Aberth sum) has a wave-uniform index, so it is read with v_readlane
//                                     into scalar registers: no LDS, no barrier, no scratch.  Every lane runs every
//                                     step; an accepted lane (and a lane >= pe) only does not take the update, so the
//                                     control flow is uniform and the loop ends on a ballot.
//   eaqhm_formant_candidates_kernel   one wave per frame: lane k judges root k, the rank of a qualifying pole is the
//                                     number of qualifying poles ahead of it, counted against the ballot mask.
//   eaqhm_formant_forward_kernel<N>   one block of 512 threads walks the T steps; thread s' scans the predecessors
//                                     through N nested loops over the slots (FmScan: the state table's own order, the
//                                     states of one prefix share its partial sum).  D of the previous step and the jump
//                                     table J (9 x 9, row and column 0 are "absent") sit in LDS, double-buffered: one
//                                     barrier per step.  The local cost and the J entry of the NEXT step are fetched before the
//                                     scan and used after it.
//   eaqhm_formant_backtrack_kernel    one wave: the first minimum of the last column, then lane 0 walks bp.
//
// The host model rounds every operation once, so nothing here may be contracted into an fma.  No atomics: every output
// word has one writer.
#include "eaqhm_common.h"
#include "eaqhm_wave.h"
#include "../../include/eaqhm_formant.h"

#pragma clang fp contract(off)

namespace eaqhm {

typedef long long i64;

constexpr int FM_WAVES = 4;                       // frames (waves) per block of the roots and candidates kernels
constexpr int FM_ITMAX = EAQHM_FORMANT_ITMAX;
constexpr int FM_KC = EAQHM_FORMANT_CAND;
constexpr int FM_THREADS = 512;                   // the forward kernel's block: one thread per state, 495 at most
constexpr int FM_JROW = FM_KC + 1;                // a row of J: absent, then the candidates

extern "C" __global__ void __launch_bounds__(64 * FM_WAVES)
    eaqhm_allpole_roots_kernel(const double* __restrict__ refl, i64 Nf, int p, double* __restrict__ roots,
                               int* __restrict__ iters) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i64 m = (i64)blockIdx.x * FM_WAVES + wave;
  if (m >= Nf) return;   // the kernel has no barrier
  const double kin = (lane >= 1 && lane <= p) ? refl[(size_t)m * p + (lane - 1)] : 0.0;
  const double a = stepup_lanes(kin, p, lane);
  const unsigned long long live = __ballot(kin != 0.0);   // bit i: k_i != 0 (bit 0 is never set)
  const int pe = __builtin_amdgcn_readfirstlane(live ? 63 - __clzll((long long)live) : 0);
  double zr = 0.0, zi = 0.0;
  int it = 0;
  if (pe > 0) {
    const double ape = wave_lane(a, pe);
    const double r0 = exp(log(fabs(ape)) / (double)pe);
    const double ang = 2.0 * M_PI * (double)lane / (double)pe + M_PI / (2.0 * (double)pe);
    double sn, cs;
    sincos(ang, &sn, &cs);
    zr = r0 * cs;
    zi = r0 * sn;
    const double tol = 8.0 * (double)pe * 0x1p-53;
    bool acc = lane >= pe;   // the lanes without a root never hold the frame up
    for (;;) {
      // one Horner pass: P, P' and the bound's sum s = sum |a_j| |z|^(pe-j)
      double pr = 1.0, pi = 0.0, dr = 0.0, di = 0.0, s = 1.0;
      const double az = sqrt(zr * zr + zi * zi);
      for (int j = 1; j <= pe; ++j) {
        const double aj = wave_lane(a, j);
        const double ndr = (dr * zr - di * zi) + pr;
        const double ndi = (dr * zi + di * zr) + pi;
        const double npr = (pr * zr - pi * zi) + aj;
        const double npi = pr * zi + pi * zr;
        dr = ndr;
        di = ndi;
        pr = npr;
        pi = npi;
        s = s * az + fabs(aj);
      }
      acc = acc || sqrt(pr * pr + pi * pi) <= tol * s;
      if (__ballot(!acc) == 0ull) break;
      if (it == FM_ITMAX) {
        it = FM_ITMAX + 1;
        break;
      }
      // N = P / P'
      const double den = dr * dr + di * di;
      const double Nr = (pr * dr + pi * di) / den, Ni = (pi * dr - pr * di) / den;
      // S = sum_{j != k} 1 / (z_k - z_j), ascending j, over the old iterate
      double Sr = 0.0, Si = 0.0;
      for (int j = 0; j < pe; ++j) {
        const double er = zr - wave_lane(zr, j), ei = zi - wave_lane(zi, j);
        const double dd = er * er + ei * ei;
        const double qr = er / dd, qi = ei / dd;
        if (j != lane) {
          Sr = Sr + qr;
          Si = Si - qi;
        }
      }
      // z -= N / (1 - N S)
      const double wr = 1.0 - (Nr * Sr - Ni * Si), wi = -(Nr * Si + Ni * Sr);
      const double wd = wr * wr + wi * wi;
      const double cr = (Nr * wr + Ni * wi) / wd, ci = (Ni * wr - Nr * wi) / wd;
      if (!acc) {
        zr = zr - cr;
        zi = zi - ci;
      }
      ++it;
    }
  }
  if (lane == 0) iters[m] = it;
  if (lane < p) {
    double* out = roots + ((size_t)m * p + lane) * 2;
    out[0] = lane < pe ? zr : 0.0;
    out[1] = lane < pe ? zi : 0.0;
  }
}

extern "C" __global__ void __launch_bounds__(64 * FM_WAVES)
    eaqhm_formant_candidates_kernel(const double* __restrict__ roots, const int* __restrict__ iters, i64 Nf, int p,
                                    double fs, double fmin, double fmax, double bmax, double* __restrict__ cand_f,
                                    double* __restrict__ cand_b, int* __restrict__ count) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i64 m = (i64)blockIdx.x * FM_WAVES + wave;
  if (m >= Nf) return;
  const bool has = lane < p;
  const double re = has ? roots[((size_t)m * p + lane) * 2] : 0.0;
  const double im = has ? roots[((size_t)m * p + lane) * 2 + 1] : 0.0;
  const double f = atan2(im, re) * fs / (2.0 * M_PI);
  const double b = -log(sqrt(re * re + im * im)) * fs / M_PI;
  const bool finished = iters[m] != FM_ITMAX + 1;
  const bool ok = has && finished && im > 0.0 && f >= fmin && f <= fmax && b <= bmax;
  const unsigned long long mask = __ballot(ok);
  int rank = 0;
  for (int j = 0; j < p; ++j) {
    const double fj = wave_lane(f, j);
    if (((mask >> j) & 1ull) && (fj < f || (fj == f && j < lane))) ++rank;
  }
  const int n = __popcll(mask), cnt = n < FM_KC ? n : FM_KC;
  if (ok && rank < FM_KC) {
    cand_f[(size_t)m * FM_KC + rank] = f;
    cand_b[(size_t)m * FM_KC + rank] = b;
  }
  if (lane < FM_KC && lane >= cnt) {
    cand_f[(size_t)m * FM_KC + lane] = NAN;
    cand_b[(size_t)m * FM_KC + lane] = NAN;
  }
  if (lane == 0) count[m] = cnt;
}

__device__ __forceinline__ int fm_count(const int* __restrict__ count, i64 t) {
  const int c = count[t];
  return c < 0 ? 0 : (c > FM_KC ? FM_KC : c);
}

// local(s, t) of the thread's own state: own[n] = s_n + 1 (0: absent)
template <int N>
__device__ __forceinline__ double fm_local(const double* __restrict__ L, const int* __restrict__ count, i64 t,
                                           const int (&own)[N], double absent) {
  const int c = fm_count(count, t);
  double acc = 0.0;
  bool bad = false;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const int idx = own[n] > 0 ? own[n] - 1 : 0;
    const double v = L[((size_t)t * N + n) * FM_KC + idx];
    bad = bad || own[n] > c;
    acc = acc + (own[n] > 0 ? v : absent);
  }
  return bad ? INFINITY : acc;
}

// J[a][b] of the step into t >= 1 (a, b = candidate index + 1; 0: absent)
__device__ __forceinline__ double fm_jump(const double* __restrict__ lf, const int* __restrict__ count, i64 t, int a,
                                          int b, double wj) {
  if (a == 0 || b == 0 || a > fm_count(count, t - 1) || b > fm_count(count, t)) return 0.0;
  return wj * fabs(lf[(size_t)t * FM_KC + (b - 1)] - lf[(size_t)(t - 1) * FM_KC + (a - 1)]);
}

// The scan of one thread over all predecessors, in state order.  The table is lexicographic, so the states are the
// leaves of N nested loops, slot 0 outermost: slot n takes "absent" (row 0 of J) first, then the candidates above the
// last one used (rows lo + 1 .. 8).  The partial slot sums are carried down the loops, so the states that share a prefix
// share its sum: each leaf costs one read of D and, on average, little more than one of J.  The sum of a leaf is still
// ((0.0 + J_0) + J_1) + .. in slot order, the bits of the plain double loop.  Every bound is the same on all threads.
template <int N, int n>
struct FmScan {
  static __device__ __forceinline__ void run(const double* const (&Jc)[N], const double* __restrict__ Dp, int lo,
                                             double acc, int& s, double& best, int& arg) {
    for (int r = 0; r <= FM_KC; r = (r == 0 ? lo + 1 : r + 1))
      FmScan<N, n + 1>::run(Jc, Dp, r == 0 ? lo : r, acc + Jc[n][r * FM_JROW], s, best, arg);
  }
};
template <int N>
struct FmScan<N, N> {
  static __device__ __forceinline__ void run(const double* const (&)[N], const double* __restrict__ Dp, int, double acc,
                                             int& s, double& best, int& arg) {
    const double cand = Dp[s] + acc;
    if (cand < best) {   // strict: the first minimum in state order
      best = cand;
      arg = s;
    }
    ++s;
  }
};

template <int N>
__global__ void __launch_bounds__(FM_THREADS)
    eaqhm_formant_forward_kernel(const double* __restrict__ L, const double* __restrict__ lf,
                                 const int* __restrict__ count, const signed char* __restrict__ states, int S, i64 T,
                                 double wj, double absent, short* __restrict__ bp, double* __restrict__ last) {
  __shared__ double D[2][FM_THREADS];
  __shared__ double J[2][FM_JROW * FM_JROW + 3];
  const int tid = threadIdx.x;
  const bool mine = tid < S;
  const int ja = tid / FM_JROW, jb = tid % FM_JROW;
  const bool jrole = tid < FM_JROW * FM_JROW;
  int own[N];
#pragma unroll
  for (int n = 0; n < N; ++n) {
    int v = mine ? (int)states[(size_t)tid * N + n] + 1 : 0;
    v = v < 0 ? 0 : (v > FM_KC ? FM_KC : v);   // a table that is not the host's stays inside J
    own[n] = v;
  }
  D[0][tid] = mine ? fm_local<N>(L, count, 0, own, absent) : INFINITY;
  D[1][tid] = INFINITY;
  if (mine) bp[tid] = (short)tid;
  double loc = 0.0, jv = 0.0;
  if (T > 1) {
    loc = fm_local<N>(L, count, 1, own, absent);
    if (jrole) jv = fm_jump(lf, count, 1, ja, jb, wj);
  }
  for (i64 t = 1; t < T; ++t) {
    const int cur = (int)(t & 1);
    if (jrole) J[cur][tid] = jv;
    __syncthreads();
    double loc_next = 0.0, jv_next = 0.0;
    if (t + 1 < T) {   // in flight during the scan
      loc_next = fm_local<N>(L, count, t + 1, own, absent);
      if (jrole) jv_next = fm_jump(lf, count, t + 1, ja, jb, wj);
    }
    const double* Dp = D[1 - cur];
    const double* Jc[N];
#pragma unroll
    for (int n = 0; n < N; ++n) Jc[n] = J[cur] + own[n];
    double best = INFINITY;
    int arg = 0, s = 0;
    FmScan<N, 0>::run(Jc, Dp, 0, 0.0, s, best, arg);   // s ends at S
    if (mine) {
      D[cur][tid] = best + loc;
      bp[(size_t)t * S + tid] = (short)arg;
    }
    loc = loc_next;
    jv = jv_next;
  }
  if (mine) last[tid] = D[(int)((T - 1) & 1)][tid];
}

extern "C" __global__ void __launch_bounds__(64)
    eaqhm_formant_backtrack_kernel(const short* __restrict__ bp, const double* __restrict__ last, int S, i64 T,
                                   int* __restrict__ q, double* __restrict__ total) {
  const int lane = threadIdx.x;
  double bv = INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < S; c += 64) {   // ascending per lane: a later state wins only with a smaller value
    const double v = last[c];
    if (bi == 0x7fffffff || v < bv) {
      bv = v;
      bi = c;
    }
  }
  for (int d = 1; d < 64; d <<= 1) {
    const double ov = __shfl_xor(bv, d);
    const int oi = __shfl_xor(bi, d);
    const bool take = ov < bv || (ov == bv && oi < bi);
    bv = take ? ov : bv;
    bi = take ? oi : bi;
  }
  if (lane != 0) return;
  int s = bi < 0 ? 0 : (bi >= S ? S - 1 : bi);
  total[0] = bv;
  q[T - 1] = s;
  for (i64 t = T - 1; t >= 1; --t) {
    s = bp[(size_t)t * S + s];
    s = s < 0 ? 0 : (s >= S ? S - 1 : s);   // a bp that is not the forward pass's stays inside the rows
    q[t - 1] = s;
  }
}
}  // namespace eaqhm

using namespace eaqhm;

static int fm_states(int N) { return N == 1 ? 9 : N == 2 ? 45 : N == 3 ? 165 : 495; }   // C(8 + N, N)

extern "C" int eaqhm_allpole_roots(eaqhm_ctx* ctx, const double* refl, int64_t Nf, int32_t p, double* roots,
                                   int32_t* iters) {
  if (!ctx) return EAQHM_EINVAL;
  if (!refl || !roots || !iters) return ctx->fail(EAQHM_EINVAL, "eaqhm_allpole_roots: bad argument");
  if (p < 1 || p > EAQHM_FORMANT_ORDER || Nf < 1 || Nf > ((int64_t)1 << 31) - 1)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_allpole_roots: need 1 <= p <= 63, 1 <= Nf < 2^31");
  hipLaunchKernelGGL(eaqhm_allpole_roots_kernel, dim3((unsigned)((Nf + FM_WAVES - 1) / FM_WAVES)), dim3(64 * FM_WAVES),
                     0, ctx->stream, refl, (i64)Nf, (int)p, roots, (int*)iters);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_formant_candidates(eaqhm_ctx* ctx, const double* roots, const int32_t* iters, int64_t Nf, int32_t p,
                                        double fs, double fmin, double fmax, double bw_max, double* cand_f,
                                        double* cand_b, int32_t* count) {
  if (!ctx) return EAQHM_EINVAL;
  if (!roots || !iters || !cand_f || !cand_b || !count)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_formant_candidates: bad argument");
  if (p < 1 || p > EAQHM_FORMANT_ORDER || Nf < 1 || Nf > ((int64_t)1 << 31) - 1 || !std::isfinite(fs) || !(fs > 0.0) ||
      !std::isfinite(fmin) || !std::isfinite(fmax) || !std::isfinite(bw_max))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_formant_candidates: need 1 <= p <= 63, 1 <= Nf < 2^31, fs > 0, finite limits");
  hipLaunchKernelGGL(eaqhm_formant_candidates_kernel, dim3((unsigned)((Nf + FM_WAVES - 1) / FM_WAVES)),
                     dim3(64 * FM_WAVES), 0, ctx->stream, roots, (const int*)iters, (i64)Nf, (int)p, fs, fmin, fmax,
                     bw_max, cand_f, cand_b, (int*)count);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

template <int N>
static hipError_t fm_launch_forward(eaqhm_ctx* ctx, const double* L, const double* lf, const int* count,
                                    const signed char* states, i64 T, double wj, double absent, short* bp, double* last) {
  hipLaunchKernelGGL(eaqhm_formant_forward_kernel<N>, dim3(1), dim3(FM_THREADS), 0, ctx->stream, L, lf, count, states,
                     fm_states(N), T, wj, absent, bp, last);
  return hipGetLastError();
}

extern "C" int eaqhm_formant_forward(eaqhm_ctx* ctx, const double* L, const double* lf, const int32_t* count,
                                     const int8_t* states, int32_t N, int64_t T, double w_jump, double absent_cost,
                                     int16_t* bp, double* last) {
  if (!ctx) return EAQHM_EINVAL;
  if (!L || !lf || !count || !states || !bp || !last)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_formant_forward: bad argument");
  if (N < 1 || N > EAQHM_FORMANT_TRACKS || T < 1 || T > ((int64_t)1 << 31) - 1 || !std::isfinite(w_jump) ||
      !(w_jump >= 0.0) || !std::isfinite(absent_cost) || !(absent_cost >= 0.0))
    return ctx->fail(EAQHM_EINVAL, "eaqhm_formant_forward: need 1 <= N <= 4, 1 <= T < 2^31, w_jump and absent_cost "
                                   "finite and >= 0");
  const signed char* st = (const signed char*)states;
  hipError_t e = N == 1   ? fm_launch_forward<1>(ctx, L, lf, (const int*)count, st, (i64)T, w_jump, absent_cost, bp, last)
                 : N == 2 ? fm_launch_forward<2>(ctx, L, lf, (const int*)count, st, (i64)T, w_jump, absent_cost, bp, last)
                 : N == 3 ? fm_launch_forward<3>(ctx, L, lf, (const int*)count, st, (i64)T, w_jump, absent_cost, bp, last)
                          : fm_launch_forward<4>(ctx, L, lf, (const int*)count, st, (i64)T, w_jump, absent_cost, bp, last);
  HIP_TRY(ctx, e);
  return EAQHM_OK;
}

extern "C" int eaqhm_formant_backtrack(eaqhm_ctx* ctx, const int16_t* bp, const double* last, int32_t N, int64_t T,
                                       int32_t* q, double* total) {
  if (!ctx) return EAQHM_EINVAL;
  if (!bp || !last || !q || !total) return ctx->fail(EAQHM_EINVAL, "eaqhm_formant_backtrack: bad argument");
  if (N < 1 || N > EAQHM_FORMANT_TRACKS || T < 1 || T > ((int64_t)1 << 31) - 1)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_formant_backtrack: need 1 <= N <= 4, 1 <= T < 2^31");
  hipLaunchKernelGGL(eaqhm_formant_backtrack_kernel, dim3(1), dim3(64), 0, ctx->stream, (const short*)bp, last,
                     fm_states((int)N), (i64)T, (int*)q, total);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
