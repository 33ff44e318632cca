// eaqhm_ls_a0tile.hip — adaptation 0 of the tile classes in a kernel of its own, two workgroups resident per CU (gfx950).
//
// The adaptation-0 frame (eaqhm_ls_a0.h: Toeplitz tables, two real systems of <= 7 tile rows side by side) has no
// contraction; a frame is a chain of dependent steps — table rotations, the diag_Dr / diag_Zr pipeline of each stage,
// two barriers per stage and per tile row of the back substitution — that leaves the pipes of its CU idle.  Inside
// eaqhm_ls_tile_kernel it inherits that kernel's registers (256 per lane) and LDS (~150 KB), so one workgroup is
// resident per CU.  Here the same frame runs with what it needs:
//   registers  __launch_bounds__(512, 4): 128 per lane, two workgroups of eight waves per CU.  The frame is three
//              noinline phases with a register allocation each (tables | fill, factorisation, back substitution |
//              record); the LDS addresses are 32-bit address_space(3) pointers, so the tile loops hold one register
//              per address and use ds_ instructions with immediate offsets;
//   LDS        W2 / PA / PB / win / sig lie inside the region the panels take over after the fill and are sized from
//              the launch's wl_max (a0res_lds_doubles, eaqhm_ls_a0.h): <= 80 KiB per workgroup.
// Same eight waves per frame, same tile ownership and helper rule, same summation orders as a0_frame<7, 7, 2>: the
// records are bit for bit those of the mode-0 branch of eaqhm_ls_tile_kernel, which stays as the path for launches
// whose LDS does not fit (and for EAQHM_OPT_A0_RESIDENT = 0).
#include "eaqhm_ls_common.h"
#include "eaqhm_ls_chol.h"
#include "eaqhm_ls_a0.h"

namespace eaqhm {

typedef __attribute__((address_space(3))) double lds_f64;
typedef __attribute__((address_space(3))) int lds_i32;
// the generic view of an LDS address for the shared helpers: they are inlined, and the compiler then sees through it
__device__ inline double* gen(lds_f64* p) { return (double*)p; }

#define A0R_THREADS 512
#define A0R_M A0_M

// the carve-up of a0res_lds_doubles(A0R_M, TZ_TB, TZ_NCH, WP, NP, .)
struct A0ResLds {
  lds_f64 *tab, *part, *Pan, *Wt, *W2, *PA, *PB, *win, *sig;
  lds_f64 *Ldl, *post, *dumpD, *zs, *zv, *xv, *dorig, *solv, *sh, *xs;
  lds_i32* flags;
};
__device__ inline A0ResLds a0res_carve(double* lds_, int WP, int NP) {
  constexpr int M = A0R_M;
  A0ResLds l;
  lds_f64* lds = (lds_f64*)(size_t)(unsigned)uni((int)(size_t)(lds_f64*)lds_);
  l.tab = lds;                                               // [TZ_NQ][TB]
  l.part = l.tab + TZ_NQ * TZ_TB;                            // [NCH][TZ_NQ][TB]
  l.W2 = l.part + TZ_NCH * TZ_NQ * TZ_TB;                    // [wl+1] each: dead with win / sig once the tables exist
  l.PA = l.W2 + WP;
  l.PB = l.PA + WP;
  l.win = l.PB + WP;                                         // [N]
  l.sig = l.win + NP;                                        // [N]
  l.Pan = lds;                                               // [2][M][TL_TILE]  panels (over all of the above, after the fill)
  l.Wt = l.Pan + 2 * M * TL_TILE;                            // [2][M][TL_TILE]  inverses of the diagonal tiles
  l.Ldl = lds + a0res_head_doubles(M, TZ_TB, TZ_NCH, WP, NP);  // [2][TL_TILE]
  l.post = l.Ldl + 2 * TL_TILE;                              // [2][8 * 32]
  l.dumpD = l.post + 2 * 256;                                // [2][64]
  l.zs = l.dumpD + 2 * 64;                                   // [2][64]
  l.zv = l.zs + 2 * 64;                                      // [2][16 * M]
  l.xv = l.zv + 2 * 16 * M;                                  // [2][16]
  l.dorig = l.xv + 2 * 16;                                   // [2][16 * M]
  l.solv = l.dorig + 2 * 16 * M;                             // [2][16 * M]   solutions of the two systems
  l.sh = l.solv + 2 * 16 * M;                                // 16
  l.flags = (lds_i32*)(l.sh + 16);                           // [2] step counters of the diagonal pipelines
  l.xs = l.sh + 18;                                          // 4 * Kcmax
  return l;
}

// ---- phase 1: window and signal into LDS, the Toeplitz tables (l.tab) and the signal energy (l.sh[0])
__device__ __attribute__((noinline)) void a0res_tables(const LsArgs& A, double* lds_, int f_, int WP_, int NP_) {
  const int f = uni(f_), tid = threadIdx.x;
  const A0ResLds l = a0res_carve(lds_, uni(WP_), uni(NP_));
  const int K = uni(A.frame_K[f]), c = uni(A.frame_c[f]), wl = uni(A.frame_wl[f]), N = 2 * wl + 1;
  const double f0 = uni(A.frame_f0[f]);
  unsigned long long* dbg = uni(A.debug);
  unsigned long long t_prev = 0;
  if (dbg && tid == 0) t_prev = __builtin_amdgcn_s_memtime();
  for (int t = tid; t < N; t += A0R_THREADS) {
    l.win[t] = window_value(1, t, N);
    l.sig[t] = uni(A.s)[(size_t)(c - wl) + t];
  }
  __syncthreads();
  LS_STAMP(0);
  toeplitz_tables(gen(l.tab), gen(l.part), gen(l.W2), gen(l.PA), gen(l.PB), gen(l.sh), gen(l.win), gen(l.sig), K, wl,
                  f0 * (2.0 * M_PI / uni(A.fs)), tid, TZ_TB, TZ_NCH, A0R_THREADS);
  LS_STAMP(1);
}

// ---- phase 2: fill, factorisation and back substitution of the two systems (a0_frame<NS, 7, 2>, statement by statement;
//      NS tiles per wave: 6 for <= 6 tile rows, 7 for 7).  Leaves the solutions in l.solv.
template <int NS>
__device__ __attribute__((noinline)) void a0res_solve(const LsArgs& A, double* lds_, int f_, int WP_, int NP_) {
  constexpr int M = A0R_M, WPS = 4;
  const int f = uni(f_);
  const int tid = threadIdx.x, lane = tid & 63, lq = lane >> 4, lcol = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wv = wave & (WPS - 1);
  const A0ResLds l = a0res_carve(lds_, uni(WP_), uni(NP_));
  const int K = uni(A.frame_K[f]), Kc = 2 * K + 1, m = (Kc + 1 + 15) >> 4, is = Kc - 16 * (m - 1), nts = m * (m + 1) / 2;
  const double ssq = l.sh[0];
  unsigned long long* dbg = uni(A.debug);
  unsigned long long t_prev = 0;
  if (dbg && tid == 0) t_prev = __builtin_amdgcn_s_memtime();

  // this wave's tiles of its system (numbered column by column, tile y on wave y % WPS, slot y / WPS)
  int tP[NS], tQ[NS];
  bool live[NS];
#pragma unroll
  for (int sl = 0; sl < NS; ++sl) {
    const int y = sl * WPS + wv;
    live[sl] = y < nts;
    int P = 0, Q = 0;
    if (live[sl]) {
      int start = 0;
      while (Q + 1 < m && start + (m - Q) <= y) { start += m - Q; ++Q; }
      P = Q + (y - start);
    }
    tP[sl] = __builtin_amdgcn_readfirstlane(P);
    tQ[sl] = __builtin_amdgcn_readfirstlane(Q);
  }

  const int sys = wave >> 2;   // which system this wave works on, and which set of work areas
  lds_f64* Pan = l.Pan + sys * M * TL_TILE;
  lds_f64* Wt = l.Wt + sys * M * TL_TILE;
  lds_f64* dorig = l.dorig + sys * 16 * M;
  lds_f64* post = l.post + sys * 256;
  lds_i32* flag = l.flags + sys;
  d4 acc[NS];
  if (tid < 2) l.flags[tid] = 0;
#pragma unroll
  for (int sl = 0; sl < NS; ++sl) {
    acc[sl] = live[sl] ? a0_entry4(gen(l.tab), TZ_TB, ssq, sys, 16 * tP[sl] + lq, 16 * tQ[sl] + lcol, K, Kc) : (d4){0, 0, 0, 0};
    if (live[sl] && tP[sl] == tQ[sl]) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (lq + 4 * r == lcol) dorig[16 * tP[sl] + lcol] = acc[sl][r];
    }
  }
  __syncthreads();   // the tables, the window and the signal are dead: their space becomes panel / inverse storage
  LS_STAMP(2);

  int* fault = uni(A.fault);
  // this lane's operand of k-step 0 of a published tile (k-step ks: + 4 ks TL_LD) and its first entry of a tile stored
  // k-major.  Opaque to the compiler inside a stage: a tile's address is then one addition where it is used — hoisted out
  // of the stage loop, the 7 x 3 addresses of a wave's tiles do not fit 128 registers beside the tiles and are spilled
  const int o0_ = lq * TL_LD + lcol, ot_ = lcol * TL_LD + lq;
#define A0R_UPDATE(sl)                                                                                        \
  {                                                                                                           \
    const lds_f64* ar = Pan + tP[sl] * TL_TILE + o0;                                                          \
    const lds_f64* br = Pan + tQ[sl] * TL_TILE + o0;                                                          \
    _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                                                          \
      acc[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[4 * ks * TL_LD], -br[4 * ks * TL_LD], acc[sl], 0, 0, 0); \
  }
  for (int jb = 0; jb < m; ++jb) {
    const int yd = jb * m - jb * (jb - 1) / 2;   // the diagonal tile of this stage
    int o0 = o0_, ot = ot_;
    asm volatile("" : "+v"(o0), "+v"(ot));
    d4 Rt = (d4){0, 0, 0, 0};
    bool mine = false;
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
      if (!live[sl] || tP[sl] != jb || tQ[sl] != jb) continue;
      if (jb > 0) A0R_UPDATE(sl)
      Rt = acc[sl];
      mine = true;
    }
    if (mine)
      diag_Dr(Rt, gen(post), (int*)flag, 16 * jb, gen(l.dumpD + sys * 64), gen(l.Ldl + sys * TL_TILE), jb == m - 1);
    LS_STAMP(10);
    if (jb > 0) {
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) {
        if (!live[sl] || tQ[sl] < jb || (tP[sl] == jb && tQ[sl] == jb)) continue;
        A0R_UPDATE(sl)
      }
    }
    // the helper wave builds the inverse after its own trailing tiles (diag_Dr's posts wait in LDS)
    if (!mine && wv == ((yd + 1) & (WPS - 1)))
      diag_Zr(gen(post), (int*)flag, 16 * jb, gen(l.zs + sys * 64), gen(Wt + jb * TL_TILE), gen(dorig + 16 * jb),
              (jb == m - 1) ? is : 16, fault);
    LS_STAMP(8);
    __syncthreads();  // (A)
    LS_STAMP(6);
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {   // panel tiles: X = T W^T, published k-major
      if (!live[sl] || tQ[sl] != jb || tP[sl] == jb) continue;
      lds_f64* tr = Pan + tP[sl] * TL_TILE;
#pragma unroll
      for (int r = 0; r < 4; ++r) tr[ot + 4 * r] = acc[sl][r];
      __builtin_amdgcn_wave_barrier();
      const lds_f64* wt = Wt + jb * TL_TILE;
      d4 x = (d4){0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) x = __builtin_amdgcn_mfma_f64_16x16x4f64(tr[o0 + 4 * ks * TL_LD], wt[o0 + 4 * ks * TL_LD], x, 0, 0, 0);
      acc[sl] = x;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int r = 0; r < 4; ++r) tr[ot + 4 * r] = x[r];
    }
    LS_STAMP(7);
    __syncthreads();  // (C)
  }
#undef A0R_UPDATE
  LS_STAMP(3);

  // ---- back substitution  L^T x = y,  y = row `is` of the last tile row
  lds_f64* zvs = l.zv + sys * 16 * M;
  lds_f64* xv = l.xv + sys * 16;
#pragma unroll
  for (int sl = 0; sl < NS; ++sl) {
    if (!live[sl] || tP[sl] != m - 1 || tQ[sl] == m - 1) continue;
    if (lq == (is & 3)) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r == (is >> 2)) zvs[16 * tQ[sl] + lcol] = acc[sl][r];
    }
  }
  if (wv == 0 && lane < 16) zvs[16 * (m - 1) + lane] = (lane < is) ? l.Ldl[sys * TL_TILE + is * TL_LD + lane] : 0.0;
  __syncthreads();
  for (int P = m - 1; P >= 0; --P) {
    {   // x_P = W_PP^T z_P: 256 threads of the system's waves, thread (i, k) one term of row i
      const int ts = tid & (64 * WPS - 1), i = (ts >> 4) & 15, k = ts & 15;
      double x = (k >= i) ? Wt[P * TL_TILE + i * TL_LD + k] * zvs[16 * P + k] : 0.0;
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) x += __shfl_xor(x, o);
      if (k == 0) {
        xv[i] = x;
        l.solv[sys * 16 * M + 16 * P + i] = x;
      }
    }
    __syncthreads();
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
      if (!live[sl] || tP[sl] != P || tQ[sl] == P) continue;
      double sr = 0;   // sum_i L[i][j] x[i] over this lane's rows i = lq + 4r
#pragma unroll
      for (int r = 0; r < 4; ++r) sr += acc[sl][r] * xv[lq + 4 * r];
      sr += __shfl_xor(sr, 16);
      sr += __shfl_xor(sr, 32);
      if (lq == 0) zvs[16 * tQ[sl] + lcol] -= sr;
    }
    __syncthreads();
  }
  LS_STAMP(4);
}

// ---- phase 3: back to the complex amplitudes and slopes in the order of the complex code, [negative | DC | positive],
//      and the record row
__device__ __attribute__((noinline)) void a0res_record(const LsArgs& A, double* lds_, int f_, int WP_, int NP_) {
  constexpr int M = A0R_M;
  const int f = uni(f_), tid = threadIdx.x;
  const A0ResLds l = a0res_carve(lds_, uni(WP_), uni(NP_));
  const int K = uni(A.frame_K[f]), Kc = 2 * K + 1;
  unsigned long long* dbg = uni(A.debug);
  unsigned long long t_prev = 0;
  if (dbg && tid == 0) t_prev = __builtin_amdgcn_s_memtime();
  const lds_f64* ev = l.solv;                      // u_0..u_K, q_1..q_K
  const lds_f64* od = l.solv + 16 * M;             // v_1..v_K, p_0..p_K
  for (int col = tid; col < Kc; col += A0R_THREADS) {
    const int h = (col < K) ? -(col + 1) : (col - K), k = (h < 0) ? -h : h;
    double ar, ai, br, bi;
    if (k == 0) { ar = ev[0]; ai = 0.0; br = od[K]; bi = 0.0; }
    else {
      ar = 0.5 * ev[k]; ai = -0.5 * od[k - 1];
      br = 0.5 * od[K + k]; bi = -0.5 * ev[K + k];
      if (h < 0) { ai = -ai; bi = -bi; }
    }
    l.xs[2 * col] = ar; l.xs[2 * col + 1] = ai;
    l.xs[2 * (Kc + col)] = br; l.xs[2 * (Kc + col) + 1] = bi;
  }
  __syncthreads();
  write_record(A, gen(l.xs), gen(l.sh), nullptr, f, K, uni(A.frame_inst[f]), uni(A.frame_c[f]), uni(A.frame_f0[f]), false);
  LS_STAMP(5);
  if (dbg && tid == 0) atomicAdd(dbg + 15, 1ull);   // frames this kernel solved (slot 15: not a stamp of a mode-0 tile launch)
}

// Persistent, frames of the tile classes 0-5 from the per-class cursors of A.cls, largest first, as in
// eaqhm_ls_tile_kernel.  A frame whose window is longer than the launch's wl_max breaks the contract of
// eaqhm_ls_batch: it is dropped and counted (fault[2]) like one whose window leaves the signal.
extern "C" __global__ void __launch_bounds__(A0R_THREADS, 4) eaqhm_ls_a0tile_kernel(LsArgs A, int WP, int NP) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int nxt;
  for (int C = LS_BIG_CLASS - 1; C >= 0; --C)
    for (;;) {
      if (threadIdx.x == 0) nxt = atomicAdd(A.cls + 8 + C, 1);
      __syncthreads();
      const int item = nxt;
      __syncthreads();
      if (item >= A.cls[C]) break;
      const int f = uni(A.cls[16 + (size_t)C * A.n_frames + item]);
      const int wl = uni(A.frame_wl[f]), m = (2 * uni(A.frame_K[f]) + 2 + 15) >> 4;   // (m <= 7: frame_class)
      if (wl + 1 > WP || 2 * wl + 1 > NP) {
        if (threadIdx.x == 0) atomicAdd(A.fault + 2, 1);
        continue;
      }
      a0res_tables(A, lds, f, WP, NP);
      if (m <= 6) a0res_solve<6>(A, lds, f, WP, NP);
      else a0res_solve<7>(A, lds, f, WP, NP);
      a0res_record(A, lds, f, WP, NP);
    }
}

// LDS bytes of a launch with these limits (the frames of the tile classes have Kc <= 103 whatever Kcmax is)
static size_t a0res_launch_bytes(const LsArgs& A, int& WP, int& NP) {
  const int wl_max = A.Nmax >> 1, Kc = A.Kcmax < 103 ? A.Kcmax : 103;
  WP = (wl_max + 8) & ~7;
  NP = (A.Nmax + 7) & ~7;
  return a0res_lds_doubles(A0R_M, TZ_TB, TZ_NCH, WP, NP, Kc) * sizeof(double);
}

// does the mode-0 launch fit two workgroups per CU?  (otherwise: the mode-0 branch of eaqhm_ls_tile_kernel)
bool ls_a0tile_fits(const LsArgs& A) {
  int WP, NP;
  return a0res_launch_bytes(A, WP, NP) <= A0RES_LDS_LIMIT;
}

// A.cls / A.debug are set by the caller (eaqhm_ls_batch), after launch_ls_prepass.
int launch_ls_a0tile(eaqhm_ctx* ctx, LsArgs A) {
  int WP, NP;
  const size_t lds_bytes = a0res_launch_bytes(A, WP, NP);
  if (lds_bytes > A0RES_LDS_LIMIT) return ctx->fail(EAQHM_EINVAL, "eaqhm_ls_batch: LDS budget exceeded (adaptation 0, resident kernel)");
  const int grid = 2 * ctx->n_cu < A.n_frames ? 2 * ctx->n_cu : A.n_frames;
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_ls_a0tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipLaunchKernelGGL(eaqhm_ls_a0tile_kernel, dim3(grid), dim3(A0R_THREADS), lds_bytes, ctx->stream, A, WP, NP);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

}  // namespace eaqhm
