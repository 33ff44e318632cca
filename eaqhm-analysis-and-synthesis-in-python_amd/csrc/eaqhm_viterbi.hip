// eaqhm_viterbi.hip — the continuous pitch track: a Viterbi decode over the SWIPE' strengths with an
// optional unvoiced state, its backtrack, and the refinement along the path.  gfx950 (MI355X) only.
//
//   eaqhm_viterbi_forward_kernel<K>   one block of 256 threads walks the T steps; thread i owns the K neighbouring
//                                     candidates K i .. K i + K - 1 (K = ceil(npc / 256)).  D of the previous step lies
//                                     in LDS between two margins of -inf (W cells, rounded up to whole batches of 8); a
//                                     step grows a register window outwards from the thread's own cells, one cell to
//                                     the left and one to the right per distance d, read eight distances at a time, so
//                                     that its K outputs share 2 W + K reads.  Each side goes through the distances in
//                                     ascending order with a strict comparison, and the right side wins only with a
//                                     larger value or an equal one nearer by: that IS the tie rule.  S is staged through LDS a tile of EAQHM_VITERBI_TILE instants at a time:
//                                     the next tile is fetched into registers when the current one begins and written
//                                     to LDS when it ends.  The same loop carries, per state, the state it descends
//                                     from at the start of the tile (an LDS gather), written once per tile.
//   eaqhm_viterbi_ends_kernel         one block: the end state from the last column, then one lane walks the tile maps
//                                     and writes the state at every tile boundary.
//   eaqhm_viterbi_fill_kernel         one lane per tile fills the tile's inner instants from the back-pointers.
//   eaqhm_viterbi_refine_kernel       one lane per instant: eaqhm_swipe_pick_kernel's arithmetic after its maximum, on
//                                     the path's candidate.
//
// The recurrence has no product; the refinement has, and the host model rounds every operation once, so nothing here
// may be contracted into an fma.  No atomics: every output word has one writer.
#include "eaqhm_common.h"
#include "eaqhm_wave.h"
#include "../../include/eaqhm_viterbi.h"

#pragma clang fp contract(off)

namespace eaqhm {

typedef long long i64;

constexpr int VT_THREADS = 256;
constexpr int VT_TILE = EAQHM_VITERBI_TILE;

constexpr int VT_CHUNK = 8;   // distances whose cells are read from LDS in one batch, ahead of their comparisons
// the margin on either side of a D row, and the cost table's length: W rounded up to whole batches (the table's tail is
// +inf, so a cell beyond W never wins)
__host__ __device__ inline int vt_margin(int W) { return (W + VT_CHUNK - 1) / VT_CHUNK * VT_CHUNK; }
__host__ __device__ inline int vt_drow(int K, int W) { return VT_THREADS * K + 2 * vt_margin(W); }
// doubles of the forward kernel's LDS: two D rows with their margins, one staged tile, the cost table, the wave maxima;
// then ints: the wave maxima's indices and two origin rows
__host__ __device__ inline size_t vt_lds_bytes(int K, int W) {
  const size_t doubles = 2 * (size_t)vt_drow(K, W) + (size_t)VT_TILE * VT_THREADS * K + (size_t)(vt_margin(W) + 1) + 8;
  const size_t ints = 8 + 2 * ((size_t)VT_THREADS * K + 2);
  return doubles * sizeof(double) + ints * sizeof(int);
}

// The barrier of a step: what the threads hand each other goes through LDS alone, so it waits for this wave's LDS
// traffic only.  __syncthreads() would also wait for the step's back-pointer stores (and the fetch of the next tile) to
// come back from memory, which nothing in the kernel reads (at 88 and 273 candidates a step measured the same either way).
__device__ inline void vt_sync_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// element e of a staged tile: candidate e / TILE, instant t0 + e % TILE (a row of S is TILE neighbouring doubles)
template <int K>
__device__ inline void vt_fetch(double (&pre)[K * VT_TILE], const double* __restrict__ S, int npc, i64 T, i64 t0, int tid) {
#pragma unroll
  for (int r = 0; r < K * VT_TILE; ++r) {
    const int e = r * VT_THREADS + tid, c = e / VT_TILE, tt = e % VT_TILE;
    pre[r] = c < npc && t0 + tt < T ? S[(size_t)c * T + t0 + tt] : 0.0;
  }
}
template <int K>
__device__ inline void vt_stage(double* __restrict__ stg, const double (&pre)[K * VT_TILE], int tid) {
#pragma unroll
  for (int r = 0; r < K * VT_TILE; ++r) {
    const int e = r * VT_THREADS + tid, c = e / VT_TILE, tt = e % VT_TILE;
    stg[tt * (VT_THREADS * K) + c] = pre[r];
  }
}

template <int K>
__global__ void __launch_bounds__(VT_THREADS)
    eaqhm_viterbi_forward_kernel(const double* __restrict__ S, int npc, i64 T, const double* __restrict__ cost, int W,
                                 int uvon, double uv, double vcost, short* __restrict__ bp, short* __restrict__ tilemap,
                                 double* __restrict__ last) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int NP = VT_THREADS * K;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int DW = vt_drow(K, W), M = vt_margin(W), c0 = tid * K, ns = npc + 1;
  double* Dp = lds;                          // [2][DW]: cell M + c holds D[c]
  double* stg = Dp + 2 * DW;                 // [TILE][NP]
  double* cs = stg + VT_TILE * NP;           // [M + 1]: cost, then +inf
  double* wmv = cs + (M + 1);                // [2][4]: the waves' maxima of D
  int* wmi = (int*)(wmv + 8);                // [2][4]
  int* org = wmi + 8;                        // [2][NP + 2]
  const i64 ntiles = (T + VT_TILE - 1) / VT_TILE;

  double pre[K * VT_TILE];
  vt_fetch<K>(pre, S, npc, T, 0, tid);
  for (int i = tid; i < 2 * DW; i += VT_THREADS) Dp[i] = -INFINITY;
  for (int i = tid; i <= M; i += VT_THREADS) cs[i] = i <= W ? cost[i] : INFINITY;
  for (int i = tid; i < 2 * (NP + 2); i += VT_THREADS) org[i] = i < NP + 2 ? i : i - (NP + 2);
  vt_stage<K>(stg, pre, tid);
  __syncthreads();

  // the wave maxima of the row just written, for the unvoiced state of the next step
  auto publish = [&](const double (&d)[K], int buf) {
    double bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < K; ++i)
      if (c0 + i < npc && (bi == 0x7fffffff || d[i] > bv)) {
        bv = d[i];
        bi = c0 + i;
      }
    wave_first_max(bv, bi);
    if (lane == 0) {
      wmv[4 * buf + wv] = bv;
      wmi[4 * buf + wv] = bi;
    }
  };

  int p = 0;   // the buffer that holds step t - 1
  double U = uv;
  {
    double d0[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const int c = c0 + i;
      d0[i] = stg[c];
      if (c < npc) {
        Dp[M + c] = d0[i];
        bp[c] = (short)c;
      }
    }
    if (tid == 0) bp[npc] = (short)npc;
    if (uvon) publish(d0, 0);
  }
  __syncthreads();

  for (i64 j = 0; j < ntiles; ++j) {
    const i64 t0 = j * VT_TILE;
    const int cols = (int)(T - t0 < VT_TILE ? T - t0 : VT_TILE);
    if (j + 1 < ntiles) vt_fetch<K>(pre, S, npc, T, t0 + VT_TILE, tid);
    for (int tt = j == 0 ? 1 : 0; tt < cols; ++tt) {
      const i64 t = t0 + tt;
      const double* base = Dp + p * DW + M + c0;
      double* cur = Dp + (1 - p) * DW + M;
      const int* orgo = org + p * (NP + 2);
      int* orgn = org + (1 - p) * (NP + 2);
      // Two chains per output, the cells on the left (with the cell itself) and those on the right, each through the
      // distances in ascending order with a strict comparison; then the right one wins only with a larger value, or an
      // equal one at a smaller distance: together the tie rule.  Two chains halve the dependent compare-select run.
      double L[K], R[K], best[K], br[K];
      int off[K], kr[K];
      const double cs0 = cs[0], sv0 = stg[tt * NP + c0];
#pragma unroll
      for (int i = 0; i < K; ++i) {
        L[i] = R[i] = base[i];
        best[i] = L[i] - cs0;
        off[i] = 0;
        br[i] = -INFINITY;
        kr[i] = 0;
      }
      for (int d0 = 1; d0 <= W; d0 += VT_CHUNK) {
        double lv[VT_CHUNK], rv[VT_CHUNK], cv[VT_CHUNK];
#pragma unroll
        for (int u = 0; u < VT_CHUNK; ++u) {   // one batch of LDS reads, none waits for a comparison
          lv[u] = base[-(d0 + u)];
          rv[u] = base[K - 1 + d0 + u];
          cv[u] = cs[d0 + u];
        }
#pragma unroll
        for (int u = 0; u < VT_CHUNK; ++u) {
          const int d = d0 + u;
#pragma unroll
          for (int i = K - 1; i > 0; --i) L[i] = L[i - 1];
          L[0] = lv[u];
#pragma unroll
          for (int i = 0; i < K - 1; ++i) R[i] = R[i + 1];
          R[K - 1] = rv[u];
#pragma unroll
          for (int i = 0; i < K; ++i) {
            const double cl = L[i] - cv[u];
            if (cl > best[i]) {
              best[i] = cl;
              off[i] = d;
            }
            const double cr = R[i] - cv[u];
            if (cr > br[i]) {
              br[i] = cr;
              kr[i] = d;
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const bool right = br[i] > best[i] || (br[i] == best[i] && kr[i] < off[i]);
        best[i] = right ? br[i] : best[i];
        off[i] = right ? kr[i] : -off[i];
      }
      int from_u = npc;   // the unvoiced state's predecessor
      double Un = U;
      if (uvon) {
        double mv = wmv[4 * p];
        int mi = wmi[4 * p];
#pragma unroll
        for (int w = 1; w < 4; ++w) {   // waves in order hold ascending candidates: the first maximum
          const double ov = wmv[4 * p + w];
          if (ov > mv) {
            mv = ov;
            mi = wmi[4 * p + w];
          }
        }
        const double enter = mv - vcost, alt = U - vcost;
        if (enter > U) {
          Un = enter;
          from_u = mi;
        }
        Un = Un + uv;
#pragma unroll
        for (int i = 0; i < K; ++i)
          if (alt > best[i]) {
            best[i] = alt;
            off[i] = npc - (c0 + i);
          }
      }
      const bool opens = tt == 0;   // this step enters a new tile: the map of the one before is complete
      short* brow = bp + (size_t)t * ns;
      short* mrow = tilemap + (size_t)(opens ? j - 1 : 0) * ns;
      double dn[K];
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const int c = c0 + i;
        dn[i] = best[i] + (i == 0 ? sv0 : stg[tt * NP + c]);
        if (c < npc) {
          const int from = c + off[i];
          const int o = orgo[from];
          cur[c] = dn[i];
          brow[c] = (short)from;
          if (opens) mrow[c] = (short)o;
          orgn[c] = opens ? c : o;
        }
      }
      if (tid == 0) {
        const int o = orgo[from_u];
        brow[npc] = (short)from_u;
        if (opens) mrow[npc] = (short)o;
        orgn[npc] = opens ? npc : o;
      }
      if (uvon) publish(dn, 1 - p);
      U = Un;
      p = 1 - p;
      vt_sync_lds();
    }
    if (j + 1 < ntiles) {
      vt_stage<K>(stg, pre, tid);
      vt_sync_lds();
    }
  }
  const int* orgo = org + p * (NP + 2);
  short* mrow = tilemap + (size_t)(ntiles - 1) * ns;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int c = c0 + i;
    if (c < npc) {
      last[c] = Dp[p * DW + M + c];
      mrow[c] = (short)orgo[c];
    }
  }
  if (tid == 0) {
    last[npc] = uvon ? U : -INFINITY;
    mrow[npc] = (short)orgo[npc];
  }
}

extern "C" __global__ void __launch_bounds__(VT_THREADS)
    eaqhm_viterbi_ends_kernel(const short* __restrict__ tilemap, const double* __restrict__ last, int npc, i64 T,
                              int* __restrict__ q) {
  __shared__ double wmv[4];
  __shared__ int wmi[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = tid; c < npc; c += VT_THREADS) {   // ascending per thread: a later candidate wins only with a larger value
    const double v = last[c];
    if (bi == 0x7fffffff || v > bv) {
      bv = v;
      bi = c;
    }
  }
  wave_first_max(bv, bi);
  if (lane == 0) {
    wmv[wv] = bv;
    wmi[wv] = bi;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < 4; ++w)
    if (wmv[w] > bv || (wmv[w] == bv && wmi[w] < bi)) {
      bv = wmv[w];
      bi = wmi[w];
    }
  int s = last[npc] > bv ? npc : bi;
  const int ns = npc + 1;
  const i64 ntiles = (T + VT_TILE - 1) / VT_TILE;
  if ((T - 1) % VT_TILE != 0) q[T - 1] = s;
  for (i64 k = ntiles - 1; k >= 0; --k) {
    s = tilemap[(size_t)k * ns + s];
    s = s < 0 ? 0 : (s > npc ? npc : s);   // a tilemap that is not the forward pass's stays inside the rows
    q[k * VT_TILE] = s;
  }
}

extern "C" __global__ void __launch_bounds__(VT_THREADS)
    eaqhm_viterbi_fill_kernel(const short* __restrict__ bp, int npc, i64 T, int* __restrict__ q) {
  const i64 k = (i64)blockIdx.x * VT_THREADS + threadIdx.x;
  const i64 b = k * VT_TILE;
  if (b >= T) return;
  const i64 e = b + VT_TILE < T - 1 ? b + VT_TILE : T - 1;   // the instant whose state the first launch wrote
  if (e <= b) return;
  const int ns = npc + 1;
  int s = q[e];
  for (i64 t = e; t > b + 1; --t) {
    s = bp[(size_t)t * ns + s];
    s = s < 0 ? 0 : (s > npc ? npc : s);
    q[t - 1] = s;
  }
}

extern "C" __global__ void __launch_bounds__(VT_THREADS)
    eaqhm_viterbi_refine_kernel(const double* __restrict__ S, const int* __restrict__ q, int npc, i64 T,
                                const double* __restrict__ pc, const double* __restrict__ ntc,
                                const double* __restrict__ nftc, const double* __restrict__ ptab,
                                const int* __restrict__ nf, int nfmax, double* __restrict__ p, double* __restrict__ s) {
  const i64 it = (i64)blockIdx.x * VT_THREADS + threadIdx.x;
  if (it >= T) return;
  const int c = q[it];
  if (c < 0 || c >= npc) {   // unvoiced
    p[it] = 0.0;
    s[it] = 0.0;
    return;
  }
  const double bv = S[(size_t)c * T + it];
  if (c == 0 || c == npc - 1) {
    p[it] = pc[c];
    s[it] = bv;
    return;
  }
  // the quadratic through the three neighbours, Newton's form turned into c2 x^2 + c1 x + c0 (eaqhm_swipe_pick_kernel)
  const double y0 = S[(size_t)(c - 1) * T + it], y2 = S[(size_t)(c + 1) * T + it];
  const double x0 = ntc[3 * (size_t)c], x1 = ntc[3 * (size_t)c + 1], x2 = ntc[3 * (size_t)c + 2];
  const double d01 = (bv - y0) / (x1 - x0), d12 = (y2 - bv) / (x2 - x1);
  const double c2 = (d12 - d01) / (x2 - x0);
  const double c1 = d01 - c2 * (x0 + x1);
  const double cc0 = y0 - x0 * (d01 - c2 * x1);
  int cnt = nf[c];
  cnt = cnt < 1 ? 1 : (cnt > nfmax ? nfmax : cnt);
  double fv = -INFINITY;
  int fi = 0;
  for (int k = 0; k < cnt; ++k) {   // ascending: the first maximum
    const double xf = nftc[(size_t)c * nfmax + k];
    const double v = (c2 * xf + c1) * xf + cc0;   // Horner, as numpy.polyval
    if (k == 0 || v > fv) {
      fv = v;
      fi = k;
    }
  }
  p[it] = ptab[(size_t)c * nfmax + fi];
  s[it] = fv;
}
}  // namespace eaqhm

using namespace eaqhm;

template <int K>
static hipError_t vt_launch_forward(eaqhm_ctx* ctx, const double* S, int npc, i64 T, const double* cost, int W, int uvon,
                                    double uv, double vcost, short* bp, short* tilemap, double* last) {
  const size_t lds = vt_lds_bytes(K, W);
  hipError_t e = hipFuncSetAttribute((const void*)eaqhm_viterbi_forward_kernel<K>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(eaqhm_viterbi_forward_kernel<K>, dim3(1), dim3(VT_THREADS), lds, ctx->stream, S, npc, T, cost, W,
                     uvon, uv, vcost, bp, tilemap, last);
  return hipGetLastError();
}

extern "C" int eaqhm_viterbi_forward(eaqhm_ctx* ctx, const double* S, int32_t npc, int64_t T, const double* cost,
                                     int32_t W, int32_t unvoiced, double uv, double vcost, int16_t* bp, int16_t* tilemap,
                                     double* last) {
  if (!ctx) return EAQHM_EINVAL;
  if (!S || !cost || !bp || !tilemap || !last) return ctx->fail(EAQHM_EINVAL, "eaqhm_viterbi_forward: bad argument");
  const int64_t lim = ((int64_t)1 << 31) - 1;
  bool ok = npc >= 3 && npc <= EAQHM_VITERBI_NPC && T >= 1 && T <= lim && W >= 0 && W <= EAQHM_VITERBI_JUMP && W <= npc - 1;
  if (unvoiced) ok = ok && std::isfinite(uv) && std::isfinite(vcost) && vcost >= 0.0;
  if (!ok)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_viterbi_forward: need 3 <= npc <= 1024, 1 <= T < 2^31, 0 <= W <= min(npc - 1, "
                                   "256), and with the unvoiced state uv finite, vcost finite and >= 0");
  const int K = (npc + VT_THREADS - 1) / VT_THREADS, on = unvoiced ? 1 : 0;
  const double u = on ? uv : 0.0, vc = on ? vcost : 0.0;
  hipError_t e = K == 1   ? vt_launch_forward<1>(ctx, S, npc, (i64)T, cost, W, on, u, vc, bp, tilemap, last)
                 : K == 2 ? vt_launch_forward<2>(ctx, S, npc, (i64)T, cost, W, on, u, vc, bp, tilemap, last)
                 : K == 3 ? vt_launch_forward<3>(ctx, S, npc, (i64)T, cost, W, on, u, vc, bp, tilemap, last)
                          : vt_launch_forward<4>(ctx, S, npc, (i64)T, cost, W, on, u, vc, bp, tilemap, last);
  HIP_TRY(ctx, e);
  return EAQHM_OK;
}

extern "C" int eaqhm_viterbi_backtrack(eaqhm_ctx* ctx, const int16_t* bp, const int16_t* tilemap, const double* last,
                                       int32_t npc, int64_t T, int32_t* q) {
  if (!ctx) return EAQHM_EINVAL;
  if (!bp || !tilemap || !last || !q) return ctx->fail(EAQHM_EINVAL, "eaqhm_viterbi_backtrack: bad argument");
  if (npc < 3 || npc > EAQHM_VITERBI_NPC || T < 1 || T > ((int64_t)1 << 31) - 1)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_viterbi_backtrack: need 3 <= npc <= 1024, 1 <= T < 2^31");
  const i64 ntiles = ((i64)T + VT_TILE - 1) / VT_TILE;
  hipLaunchKernelGGL(eaqhm_viterbi_ends_kernel, dim3(1), dim3(VT_THREADS), 0, ctx->stream, (const short*)tilemap, last,
                     (int)npc, (i64)T, (int*)q);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(eaqhm_viterbi_fill_kernel, dim3((unsigned)((ntiles + VT_THREADS - 1) / VT_THREADS)),
                     dim3(VT_THREADS), 0, ctx->stream, (const short*)bp, (int)npc, (i64)T, (int*)q);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

extern "C" int eaqhm_viterbi_refine(eaqhm_ctx* ctx, const double* S, const int32_t* q, int32_t npc, int64_t T,
                                    const double* pc, const double* ntc, const double* nftc, const double* ptab,
                                    const int32_t* nf, int32_t nfmax, double* p, double* s) {
  if (!ctx) return EAQHM_EINVAL;
  if (!S || !q || !pc || !ntc || !nftc || !ptab || !nf || !p || !s)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_viterbi_refine: bad argument");
  if (npc < 3 || npc > EAQHM_VITERBI_NPC || T < 1 || T > ((int64_t)1 << 31) - 1 || nfmax < 1 || nfmax > 64)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_viterbi_refine: need 3 <= npc <= 1024, 1 <= T < 2^31, 1 <= nfmax <= 64");
  hipLaunchKernelGGL(eaqhm_viterbi_refine_kernel, dim3((unsigned)((T + VT_THREADS - 1) / VT_THREADS)), dim3(VT_THREADS),
                     0, ctx->stream, S, (const int*)q, (int)npc, (i64)T, pc, ntc, nftc, ptab, (const int*)nf, (int)nfmax,
                     p, s);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}
