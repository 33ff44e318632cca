// eaqhm_ls_tile.hip — the per-frame LS entirely on chip: Gramian AND factorisation on the FP64 matrix cores,
// the system matrix never leaves the register file (gfx950).
//
// A workgroup of 512 threads (8 waves, every wave owns system tiles in its registers) works on one frame at a
// time; frames are bucketed by size on the device and handed out by per-class atomic cursors, largest first.
//
// Stacked basis.  With Y[t] = w_t * [ E2(t) | n_t E2(t) | s_t ]  (2Kc+1 columns; E2 = [negative | DC | positive]
// columns of functions.py:516-519, w the analysis window, n_t = t - mid) the normal equations of
// functions.py:521-530 are the leading 2Kc x 2Kc block of  Y^H Y  and the right-hand side is its last column.
// Factorising  Y^H Y  WITH that last row/column leaves conj(L^-1 rhs) in the last row: the forward substitution
// costs nothing.  Every 16x16 complex tile of Y^H Y is one MFMA accumulation over time, owned by one wave
// (tiles numbered column by column, tile x -> wave x%8, slot x/8) from the first sample to the last back-substitution step.
//
//   A1     per-slot set-up: zero-count look-ups decide whether the slot's window has a gap; gap-free slots need
//          only their centre values, the others are bridged into per-workgroup scratch rows
//   A3+B   chunks of 16 sample PAIRS (mid-d-1, mid+d), centre outwards, built in LDS by all threads: track values
//          loaded directly, phase = running sum (16-lane DPP scan + per-slot carry); the pair shares its sincos
//          because the negative-frequency column at u is the time-reversed positive one (functions.py:284-285);
//          contracted with v_mfma_f64_16x16x4_f64, LDS operand reads software-pipelined one k-step ahead; frames of
//          <= 12 tile rows: only X = w [E2 | s] in the chunk, three-weight Gramian G_p = X^H diag(n^p) X (TW in tile_frame;
//          11-12 tile rows: dealt out by the unit tables of eaqhm_ls_twunits.h, UA / UB / TB in tile_frame; 11 tile rows with
//          the part-filled last basis tile column packed as [x_e | n x_e])
//   B0     adaptation 0: no basis at all — the Gramian in closed form from Toeplitz tables, then two real systems of
//          half the order factorised side by side (a0_frame, eaqhm_ls_a0.h).  A mode-0 launch whose LDS fits twice into
//          a CU goes to eaqhm_ls_a0tile_kernel instead (eaqhm_ls_a0tile.hip: the same frame, two workgroups per CU)
//   C      right-looking tile Cholesky with look-ahead, 2 workgroup barriers per tile row: trailing update with the
//          previous panel (the next diagonal tile first); its owner wave factorises that tile on the matrix cores
//          (diag_D: 2x2 block pivots, one rank-2 MFMA per plane and step, rows handed round by ds_bpermute) while a
//          second wave follows one step behind and builds the inverse (diag_Z) and the others finish their updates;
//          panel tiles are multiplied by the inverse (MFMA) and published in LDS; no global memory traffic
//   C'     back substitution from the L tiles still sitting in the owners' registers; z, x vectors in LDS
//   D      frequency mismatch, acceptance, record row (eaqhm_ls_common.h)
//
// Frames with more than 13 tile rows (Kc > 103) do not fit the register budget and are left to
// eaqhm_ls_mfma_kernel (same Gramian, factorisation through scratch memory).
#include <type_traits>
#include "eaqhm_ls_common.h"
#include "eaqhm_ls_chol.h"
#include "eaqhm_ls_a0.h"
#include "eaqhm_ls_tilemap.h"
#include "eaqhm_ls_twunits.h"
#include "eaqhm_ls_gather.h"
#include "eaqhm_ls_tilelds.h"
#include "eaqhm_ls_tilexch.h"

namespace eaqhm {
bool ls_a0tile_fits(const LsArgs& A);                 // eaqhm_ls_a0tile.hip
int launch_ls_a0tile(eaqhm_ctx* ctx, LsArgs A);

// wave that owns the diagonal tile (jb, jb): see the ownership rules in tile_frame
#define DIAG_OWNER(jb, nt) ((int)TL_DIAG[nt][jb])
#define TL_THREADS 512
#define TL_WAVES 8
#define TL_CW 8         // all waves own tiles
// (TL_NTMAX, CI_STRIDE, CI_NCH, TL_NSLOT and the LDS budget: eaqhm_ls_tilelds.h)
static_assert(TLL_TILE == TL_TILE && TLL_DG_TILE == DG_TILE, "eaqhm_ls_tilelds.h and eaqhm_ls_chol.h disagree");
static_assert(TX_DFLAG_BYTE == 8 * (4 * TL_NTMAX * TL_TILE + 2 * TL_TILE + DGP_DOUBLES + 128 + 256), "eaqhm_ls_tilexch.h: where tile_frame puts dflag");
// (adaptation 0: closed-form Gramian and two real systems — A0_NS, A0_M, TZ_TB, TZ_NCH and a0_frame in eaqhm_ls_a0.h)

// The next frame's header, by one wave (see TlHead); the barrier that follows publishes it.
__device__ inline void fetch_next_header(const LsArgs& A, TlHead* hd, int C, int nbuf, int lane) {
  int* cls = uni(A.cls);
  int item = 0;
  if (lane == 0) item = atomicAdd(cls + 8 + C, 1);
  item = uni(item);
  int f = -1;
  if (item < uni(cls[C])) f = uni(cls[16 + (size_t)C * uni(A.n_frames) + item]);
  if (f >= 0) {
    const int* tab = (lane == 0) ? A.ncol : (lane == 1) ? A.frame_c : (lane == 2) ? A.frame_wl : A.frame_inst;
    if (lane < 4) (&hd->n)[lane] = tab[f];
    const int Kmax = uni(A.Kmax);
    if (lane < TL_NSLOT && lane < Kmax) hd->cols[nbuf][lane] = A.cols[(size_t)f * Kmax + lane];   // (the frame's row of `cols` has Kmax entries)
  }
  if (lane == 0) { hd->f = f; hd->buf = nbuf; hd->cls = C; }
}

// One frame with NS tiles per wave.  Not inlined: each register budget gets its own register allocation (inlining
// the five budgets into one kernel body spills several hundred VGPRs).
// TW = 0: the Gramian is contracted tile by tile from the stacked basis Y.  TW > 0: three-weight Gramian — the basis
// chunk holds only X = w [E2 | s] (Kc + 1 columns, T = ceil((Kc + 1) / 16) tile columns), each wave contracts at most TW
// lower-triangle pairs (I, J) of them into G_p = X_I^H diag(n^p) X_J, p = 0, 1, 2, and the system tiles of Y^H Y are
// gathered from the G_p afterwards (see the comment at the gather).
// One k-step of the three-weight contraction of a basis pair: a = X_I, b = X_J (this lane's row k), nk = n_k of that
// row.  Three real products per complex one for each of G0 = a^H b, G1 = (n a)^H b, G2 = (n a)^H (n b):
// g[3p] = re re', g[3p+1] = im im', g[3p+2] = (re + im)(im' - re')  ->  Re = g[3p] + g[3p+1], Im = g[3p+2] + g[3p] - g[3p+1]
__device__ inline void tw_step(d4 (&g)[9], double aR, double aI, double bR, double bI, double nk) {
  const double sA = aR + aI, dB = bI - bR;
  const double naR = nk * aR, naI = nk * aI, nsA = nk * sA;
  const double nbR = nk * bR, nbI = nk * bI, ndB = nk * dB;
  g[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bR, g[0], 0, 0, 0);
  g[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, bI, g[1], 0, 0, 0);
  g[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(sA, dB, g[2], 0, 0, 0);
  g[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(naR, bR, g[3], 0, 0, 0);
  g[4] = __builtin_amdgcn_mfma_f64_16x16x4f64(naI, bI, g[4], 0, 0, 0);
  g[5] = __builtin_amdgcn_mfma_f64_16x16x4f64(nsA, dB, g[5], 0, 0, 0);
  g[6] = __builtin_amdgcn_mfma_f64_16x16x4f64(naR, nbR, g[6], 0, 0, 0);
  g[7] = __builtin_amdgcn_mfma_f64_16x16x4f64(naI, nbI, g[7], 0, 0, 0);
  g[8] = __builtin_amdgcn_mfma_f64_16x16x4f64(nsA, ndB, g[8], 0, 0, 0);
}

// A whole pair in K3 slots: tw_step on three accumulator triples.
__device__ inline void twu_pair_k3(d4 (&g0)[3], d4 (&g1)[3], d4 (&g2)[3], double aR, double aI, double bR, double bI, double nk) {
  const double sA = aR + aI, dB = bI - bR;
  const double naR = nk * aR, naI = nk * aI, nsA = nk * sA;
  const double nbR = nk * bR, nbI = nk * bI, ndB = nk * dB;
  g0[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bR, g0[0], 0, 0, 0);
  g0[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, bI, g0[1], 0, 0, 0);
  g0[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(sA, dB, g0[2], 0, 0, 0);
  g1[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(naR, bR, g1[0], 0, 0, 0);
  g1[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(naI, bI, g1[1], 0, 0, 0);
  g1[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(nsA, dB, g1[2], 0, 0, 0);
  g2[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(naR, nbR, g2[0], 0, 0, 0);
  g2[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(naI, nbI, g2[1], 0, 0, 0);
  g2[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(nsA, ndB, g2[2], 0, 0, 0);
}
// A whole pair in two-accumulator slots: g[0] = re re' + im im', g[1] = re im' (- im re' with k4: form K4; without: form H,
// the diagonal pair's RI).  Four scaled operands, no sums.
__device__ inline void twu_pair_2acc(d4 (&g0)[2], d4 (&g1)[2], d4 (&g2)[2], double aR, double aI, double bR, double bI, double nk,
                                     bool k4) {
  const double naR = nk * aR, naI = nk * aI, nbR = nk * bR, nbI = nk * bI;
  g0[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bR, g0[0], 0, 0, 0);
  g1[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(naR, bR, g1[0], 0, 0, 0);
  g2[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(naR, nbR, g2[0], 0, 0, 0);
  g0[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bI, g0[1], 0, 0, 0);
  g1[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(naR, bI, g1[1], 0, 0, 0);
  g2[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(naR, nbI, g2[1], 0, 0, 0);
  g0[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, bI, g0[0], 0, 0, 0);
  g1[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(naI, bI, g1[0], 0, 0, 0);
  g2[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(naI, nbI, g2[0], 0, 0, 0);
  if (k4) {
    const double maI = -aI, mnaI = -naI;
    g0[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(maI, bR, g0[1], 0, 0, 0);
    g1[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(mnaI, bR, g1[1], 0, 0, 0);
    g2[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(mnaI, nbR, g2[1], 0, 0, 0);
  }
}

// An edge pair of a packed table, in two-accumulator slots (form K4): a = E = [x_e | n x_e] is never scaled, b = X_J for
// q = 0 (g0) and n X_J for q = 1 (g1).
__device__ inline void twu_edge_k4(d4 (&g0)[2], d4 (&g1)[2], double aR, double aI, double bR, double bI, double nk) {
  const double nbR = nk * bR, nbI = nk * bI, maI = -aI;
  g0[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bR, g0[0], 0, 0, 0);
  g1[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, nbR, g1[0], 0, 0, 0);
  g0[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bI, g0[1], 0, 0, 0);
  g1[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, nbI, g1[1], 0, 0, 0);
  g0[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, bI, g0[0], 0, 0, 0);
  g1[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, nbI, g1[0], 0, 0, 0);
  g0[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(maI, bR, g0[1], 0, 0, 0);
  g1[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(maI, nbR, g1[1], 0, 0, 0);
}

// UA + UB > 0 (TW = 0): the three-weight Gramian of a frame with TWU_TT[TB] basis tile columns, dealt out by unit table TB
// (eaqhm_ls_twunits.h: a unit is one tile G_p[I][J]).  A wave has UA slots of three accumulators (form K3: the three real
// products of tw_step) and UB slots of two (K4: four real products, re re' + im im' and re im' - im re'; H, diagonal pairs
// only: the K4 form without its fourth product, the second accumulator holds RI = sum re im' and the gather takes
// Im = RI - RI^T).  3 UA + 2 UB accumulators per wave whatever the number of basis pairs; the first 3 (UA / 3) and
// 3 (UB / 3) slots hold whole pairs, contracted like a pair of the TW form, the others single units.
// Packed tables (TWU_PACKED[TB]; classes whose last basis tile column E = T - 1 has at most 8 live columns): the chunk holds
// that tile column as [x_e | n x_e], so E^H X_J carries weights 0 and 1 of the pair (E, J) in its upper and lower eight rows
// and E^H (n X_J) weights 1 and 2 — two edge units in place of three — and the corner E^H E, one H unit, all three.
// f_ >= 0: the frame, fetched by the caller (who set buf = 1 in the workgroup's TlHead).  f_ < 0: the frame whose header
// the previous one left there.  The frame's class, whose cursor the next header is drawn from, is the one that runs this register budget.
template <int NS, int TW, int UA = 0, int UB = 0, int TB = 0>
__device__ __attribute__((noinline)) void tile_frame(const LsArgs& A, int TS_, int ldx_max_, double* lds, int f_) {
  constexpr int C = NS == 12 ? 5 : NS == 10 ? 4 : NS == 9 ? 3 : NS == 7 ? 2 : NS == 6 ? 1 : 0;   // (RUN_CLASS in the kernel)
  static_assert(NS == 12 || NS == 10 || NS == 9 || NS == 7 || NS == 6 || NS == 5, "a register budget per class");
  // What each budget keeps of the serial-phase changes is what its class gained by more than three times the run-to-run
  // spread (profiles/serial_phases): the next frame's header everywhere but at 12 tile rows, the record row
  // in LDS at 11 tile rows only.
  constexpr bool NEXT_HEAD = NS != 10, REC_ROW = NS == 9;
  const bool pre = uni(f_) < 0;
  const int TS = uni(TS_), ldx_max = uni(ldx_max_);
  const int tid = threadIdx.x, nt_thr = TL_THREADS;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // ---- LDS carve-up: region U is the basis chunk (+ slot info) in the Gramian phase, tile storage afterwards
  double* U = uni(lds);
  TlHead* hd = (TlHead*)(U + tl_head_offset());      // (behind the tile storage: xv + 32 below)
  const int f = pre ? uni(hd->f) : uni(f_);
  double* Xre = U;
  double* Xim = Xre + (size_t)TS * ldx_max;
  const size_t usize_g = (size_t)2 * TS * ldx_max;
  double* ci = U + usize_g;                          // [52][CI_STRIDE]
  unsigned long long* masks = (unsigned long long*)(ci + (size_t)CI_STRIDE * 52);  // [52][16]  (n <= 51 for Kc <= 103)
  double* PanR = U;                                  // [NT][TILE]  published panel tiles, [k][row]
  double* PanI = PanR + TL_NTMAX * TL_TILE;
  double* WtR = PanI + TL_NTMAX * TL_TILE;           // [NT][TILE]  (W^H)[k][j] of every diagonal tile
  double* WtI = WtR + TL_NTMAX * TL_TILE;
  double* LdR = WtI + TL_NTMAX * TL_TILE;            // [TILE]      last diagonal factor, [row][col]
  double* LdI = LdR + TL_TILE;
  double* Dc = LdI + TL_TILE;                        // [DG_TILE]   diagonal tile being factorised (complex, rows DG_LD apart)
  double* Zc = Dc + DG_TILE;                         // [DG_TILE]   its inverse in the making
  double* zv = Zc + DG_TILE;                        // 2*16*NT
  double* xv = zv + 2 * 16 * TL_NTMAX;               // 2*16
  double* xs = xv + 32 + TL_HEAD_DOUBLES;            // 4*Kcmax   solution in natural order
  double* sh = xs + 4 * uni(A.Kcmax);                // 16
  double* win = sh + 16;                             // [64*CI_NCH] analysis window of the frame
  double* sig = win + 64 * CI_NCH;                   // [64*CI_NCH] signal window of the frame
  double* dorig = sig + 64 * CI_NCH;                 // [16*NT]     original diagonal of the system (singularity check)

  const int Npad = ((uni(A.Nmax) + 63) >> 6) << 6;
  double* Qs = uni(A.scratch) + (size_t)blockIdx.x * (size_t)uni((int)A.scratch_stride);  // bridged fm[j][t]
  double* Rs = Qs + (size_t)Npad * uni(A.nmax);                                           // bridged am[j][t]
  const bool seeds = uni(hd->seeds) != 0;            // (A.any_seed && *A.any_seed != 0, read once by the kernel)
  // phases are q * (2 pi / fs) here, (2 pi q) / fs in the reference (functions.py:513, :453): one rounding each way,
  // <= 2 ulp of the phase apart, and no IEEE division per basis sample
  const double w1 = uni(2.0 * M_PI / A.fs);
  const int PE = TS / 2;
  const double* sA = uni(A.s);
  const int lcol = lane & 15, lq = lane >> 4;
  unsigned long long* dbg = uni(A.debug);
  unsigned long long t_prev = 0;

  {
    const int n = pre ? uni(hd->n) : uni(A.ncol[f]);
    const int Kc = 2 * n + 1, Ms = 2 * Kc + 1;   // stacked columns incl. the signal
    const int nt = (Ms + 15) >> 4;
    const int c = pre ? uni(hd->c) : uni(A.frame_c[f]), wl = pre ? uni(hd->wl) : uni(A.frame_wl[f]);
    const int inst = pre ? uni(hd->inst) : uni(A.frame_inst[f]);
    const int N = 2 * wl + 1, mid = wl;
    const int T = (Kc + 16) >> 4;                      // three-weight basis: tile columns of X = w [E2 | s]
    constexpr int UN = UA + UB;                        // unit slots of a wave
    constexpr int GA = UA / 3, GB = UB / 3;            // ... of which 3 GA + 3 GB hold whole pairs (weights 0, 1, 2 in a row)
    constexpr bool G3 = TW > 0 || UN > 0;              // three-weight Gramian (whole pairs or units)
    // The G_p tiles change hands in LDS (eaqhm_ls_tilexch.h) where whole pairs are contracted, T <= 5: the budgets of <= 10
    // tile rows.  The unit tables (T = 6: one plane per round) keep the workgroup's scratch area: their budgets are the
    // ones that spill already, and through three rounds the accumulators of the planes still to be stored stay live beside
    // the gathered system tiles.
    constexpr bool LDS_XCH = TW > 0;
    static_assert(TW == 0 || UN == 0, "whole pairs or units");
    static_assert(UN == 0 || (UA == TWU_UA && UB == TWU_UB), "slot layout of eaqhm_ls_twunits.h");
    static_assert(TB >= 0 && TB < TWU_NTB, "unit table");
    constexpr bool PK = UN > 0 && TWU_PACKED[TB];      // last basis tile column packed: [x_e | n x_e]
    constexpr int EC = 16 * (TWU_TT[TB] - 1);          // ... its first basis column (the caller picks the table by T)
    const int nb = G3 ? T : nt;                        // tile columns of the basis chunk
    const int ldx = (nb << 4) + ((nb & 1) ? 0 : 16);  // ≡ 16 (mod 32): MFMA operand reads hit disjoint bank halves
    const int npair = T * (T + 1) / 2;
    const int is = 2 * Kc - 16 * (nt - 1);  // position of the signal column inside the last tile row (2,6,10,14)
    const double f0 = uni(A.f0_stale);
    const int* mycols = pre ? (const int*)hd->cols[uni(hd->buf)] : uni(A.cols) + (size_t)f * uni(A.Kmax);
    const int npairs = mid + 1;  // pairs e = 0..mid: (u, v) = (e-1, N-1-e)

    if (dbg && tid == 0) {   // slot 11: from the previous frame's last stamp to here (the hand-out, the call, the header)
      t_prev = __builtin_amdgcn_s_memtime();
      if (hd->t_last && !uni((int)A.debug_diag)) atomicAdd(dbg + 11, t_prev - hd->t_last);
    }
    // The signal window is requested first and stored last: its round trip runs under the window values and the zeroing.
    // No barrier of its own: prepare_slots writes none of this and ends on a barrier.
    double sv[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int t = tid + r * nt_thr;
      sv[r] = (t < N) ? sA[(size_t)(c - wl) + t] : 0.0;
    }
    // region U may hold tiles of the previous frame: make the basis chunk finite and its padding zero — the TS x ldx
    // cells of either plane that this frame's class writes and reads
    for (int q = tid; q < TS * ldx; q += nt_thr) { Xre[q] = 0.0; Xim[q] = 0.0; }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int t = tid + r * nt_thr;
      if (t < N) { win[t] = window_value(false, t, N); sig[t] = sv[r]; }
    }
    int* gappy = (int*)(masks + (size_t)52 * CI_NCH);   // [52] flags
    prepare_slots<CI_STRIDE, TL_WAVES>(A, Qs, Rs, Npad, ci, masks, gappy, mycols, n, N, mid, c, wl, seeds, lane, wave, CI_NCH,
                                       REC_ROW ? hd->fmc : nullptr);
    LS_STAMP(0);

    // system tiles of this wave
    // Three real products per complex one need a third accumulator per tile: the first NM3 tiles of a wave.  Register
    // budget: every tile of the small frames, none beyond 7 slots (tried: 6 of 9 and 4 of 10 slots, 192 accumulator
    // VGPRs like the 12-slot budget — the extra spills cost more than the 17 % / 10 % fewer MFMAs gain: 1.23 M vs
    // 1.27 M frames/s on the 60 s workload).
    constexpr int NM3 = (NS <= 7) ? NS : 0;
    d4 accR[NS], accI[NS], acc3[NM3 ? NM3 : 1];
    int tP[NS], tQ[NS];
    bool live[NS];
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
      accR[sl] = (d4){0, 0, 0, 0};
      accI[sl] = (d4){0, 0, 0, 0};
      if (sl < NM3) acc3[sl] = (d4){0, 0, 0, 0};
      // Ownership: TL_MAP (eaqhm_ls_tilemap.h, generated by tools/tile_map_search.py) — the wave that owns diagonal tile jb
      // holds few tiles of the trailing matrix of stage jb, so that after diag_D it does not keep the others waiting at the
      // stage barrier with trailing tiles of its own; at most NS tiles per wave, tile counts per SIMD equal to within one
      // (the contraction stays balanced), at most ... panel tiles of a column on one wave.  (Rounds 1-2 dealt the tiles
      // out column by column, tile x on wave x % 8.)
      const int code = TL_MAP[nt][wave][sl];
      live[sl] = code != 0xFF;
      const int P = live[sl] ? (code >> 4) : 0, Q = live[sl] ? (code & 15) : 0;
      tP[sl] = __builtin_amdgcn_readfirstlane(P);   // wave-uniform: scalar registers, not spill slots
      tQ[sl] = __builtin_amdgcn_readfirstlane(Q);
    }

    // three-weight Gramian: basis pair x = wave + 8 slot (pairs numbered row by row, I >= J): pair counts per SIMD
    // (waves w and w + 4) equal to within one
    // T = 4 (ten pairs; pairs 8 and 9 whole in the second slot of waves 0 and 1 would be 27 / 27 / 18 / 18 MFMAs per k-step
    // on the four SIMDs): the second slot of waves 0..3 takes half of pair 8 (waves 0, 1) or of pair 9 (waves 2, 3) — wave
    // 2 h + b the k-steps 4 b .. 4 b + 3 of every chunk — 22.5 per SIMD.  The two partial tiles of a split pair are added
    // in a fixed order before the gather (first half + second half).
    constexpr int TWA = TW ? TW : 1;
    const bool split = TW > 0 && NS == 5 && T == 4;
    d4 g[TWA][9];
    int gI[TWA], gJ[TWA], gx[TWA];
    bool glive[TWA];
#pragma unroll
    for (int sl = 0; sl < TWA; ++sl) {
      const int x = (split && sl == 1) ? 8 + (wave >> 1) : wave + 8 * sl;
      glive[sl] = TW && x < npair && !(split && sl == 1 && wave >= 4);
      gx[sl] = __builtin_amdgcn_readfirstlane(x);
      int I = 0, J = 0;
      if (glive[sl]) tile_of(x, I, J);
      gI[sl] = __builtin_amdgcn_readfirstlane(I);
      gJ[sl] = __builtin_amdgcn_readfirstlane(J);
#pragma unroll
      for (int p = 0; p < 9; ++p) g[sl][p] = (d4){0, 0, 0, 0};
    }

    // unit slots: the first UA with three accumulators, the others with two; code as in TWU_MAPS, wave-uniform
    constexpr int UAA = UA > 3 ? UA : 3, UBA = UB > 3 ? UB : 3;   // (at least one whole pair: the unused ones cost nothing)
    d4 ga[UAA][3], gb[UBA][2];
    int ucode[UN ? UN : 1];
    if constexpr (UN > 0) {
#pragma unroll
      for (int sl = 0; sl < UN; ++sl) ucode[sl] = __builtin_amdgcn_readfirstlane((int)TWU_MAPS[TB][wave][sl]);
#pragma unroll
      for (int sl = 0; sl < UA; ++sl)
#pragma unroll
        for (int p = 0; p < 3; ++p) ga[sl][p] = (d4){0, 0, 0, 0};
#pragma unroll
      for (int sl = 0; sl < UB; ++sl) gb[sl][0] = gb[sl][1] = (d4){0, 0, 0, 0};
    }

    // ================= Gramian =================
    // sample pairs (u, v) = (mid-d-1, mid+d), d = 0..mid, taken from the centre outwards so that the phase
    // integral of functions.py:508-515 relative to the centre is a running sum
    for (int d0 = 0; d0 < npairs; d0 += PE) {
      // logical column cc of chunk rows (2*el, 2*el+1) lives at XCOL(cc, el): the 16 lanes that write one column
      // of 16 different pairs hit 16 different banks, and MFMA operand reads stay conflict-free
#pragma clang loop unroll(disable)
      for (int idx = tid; idx < 16 * n; idx += nt_thr) {
        const int el = idx & 15, j = idx >> 4, d = d0 + el;
        const bool act = d <= mid;
        const int u = mid - d - 1, v = mid + d;
        double su = 0, cu = 1, sv, cv;
        double pur = 0, pui = 0, nur = 0, nui = 0, pvr, pvi, nvr, nvi;  // positive / negative column values
        {
          double* cj = ci + j * CI_STRIDE;
          const double* fb = ((const double**)cj)[2];   // bridged copy or the track itself (prepare_slots)
          const double* ab = ((const double**)cj)[3];
          // every load of the item up front, indices clamped into the window (results of clamped ones unused)
          const int dc = act ? d : mid;
          const double fu1 = fb[mid - dc], fv = fb[mid + dc];
          const double au = ab[(mid - dc - 1 >= 0) ? (mid - dc - 1) : 0], au1 = ab[mid - dc];
          const double av = ab[mid + dc], av1 = ab[(mid + dc + 1 < N) ? (mid + dc + 1) : (N - 1)];
          // F(v) - F(mid) = sum of fm over (mid, v];  F(u) - F(mid) = -sum over [u+1, mid]
          const double xu = act ? fu1 : 0.0, xv = (act && d >= 1) ? fv : 0.0;
          const double qv = cj[0] + scan16(xv), qu = -(cj[1] + scan16(xu));
          if (el == 15) { cj[0] = qv; cj[1] = -qu; }   // carried to the next chunk (read again after two barriers)
          if (!act) continue;
          const double ainv = cj[17], pr = cj[18], pi = cj[19];
          sincos_cw(qu * w1, &su, &cu);
          sincos_cw(qv * w1, &sv, &cv);
          const double eps = 10e-5;
          // positive column at t uses E1(t); negative column at t uses ratio[mirror+1] * E1(mirror) * rho
          if (u >= 0) {
            const double ru = (eps + au) * ainv, rv1 = (eps + av1) * ainv;
            pur = ru * cu;                    pui = ru * su;
            nur = rv1 * (cv * pr - sv * pi);  nui = rv1 * (cv * pi + sv * pr);
          }
          const double rv = (eps + av) * ainv, ru1 = (eps + au1) * ainv;
          pvr = rv * cv;                      pvi = rv * sv;
          nvr = ru1 * (cu * pr - su * pi);    nvi = ru1 * (cu * pi + su * pr);
        }
        double* xr = Xre + (2 * el) * ldx;
        double* xi = Xim + (2 * el) * ldx;
        const int cpos = XCOL(n + 1 + j, el), cneg = XCOL(j, el);               // amplitude columns
        const int spos = XCOL(Kc + n + 1 + j, el), sneg = XCOL(Kc + j, el);     // slope columns (n_t times)
        const double wv = win[v], nv = (double)(v - mid);
        if (u >= 0) {
          const double wu = win[u], nu = (double)(u - mid);
          pur *= wu; pui *= wu; nur *= wu; nui *= wu;
          xr[cpos] = pur;      xi[cpos] = pui;      xr[cneg] = nur;      xi[cneg] = nui;
          if (!G3) { xr[spos] = nu * pur; xi[spos] = nu * pui; xr[sneg] = nu * nur; xi[sneg] = nu * nui; }
          if (PK && n + 1 + j >= EC) { xr[XCOL(n + 9 + j, el)] = nu * pur; xi[XCOL(n + 9 + j, el)] = nu * pui; }   // packed half
        }
        pvr *= wv; pvi *= wv; nvr *= wv; nvi *= wv;
        xr += ldx; xi += ldx;
        xr[cpos] = pvr;      xi[cpos] = pvi;      xr[cneg] = nvr;      xi[cneg] = nvi;
        if (!G3) { xr[spos] = nv * pvr; xi[spos] = nv * pvi; xr[sneg] = nv * nvr; xi[sneg] = nv * nvi; }
        if (PK && n + 1 + j >= EC) { xr[XCOL(n + 9 + j, el)] = nv * pvr; xi[XCOL(n + 9 + j, el)] = nv * pvi; }
      }
      // DC / signal columns: one thread per chunk row, spread over the waves (lanes 0, 16, 32, 48)
      if ((tid & 15) == 0 && (tid >> 4) < TS) {
        const int row = tid >> 4;
        const int d = d0 + (row >> 1);
        const int t = (row & 1) ? (mid + d) : (mid - d - 1);
        const bool ok = (d <= mid) && (t >= 0);
        const double w = ok ? win[t] : 0.0;
        const double sval = ok ? sig[t] : 0.0;
        const double nn = (double)(t - mid);
        const int el = row >> 1;
        double* xr = Xre + row * ldx;
        double* xi = Xim + row * ldx;
        xr[XCOL(n, el)] = w;               xi[XCOL(n, el)] = 0.0;            // DC column
        if (!G3) {
          xr[XCOL(Kc + n, el)] = w * nn;   xi[XCOL(Kc + n, el)] = 0.0;       // its slope copy
        }
        const int scol = G3 ? Kc : 2 * Kc;
        xr[XCOL(scol, el)] = w * sval;     xi[XCOL(scol, el)] = 0.0;         // signal column
        // packed half: weight 1 of the right-hand side's slope entries is read from the n-scaled signal's rows
        if (PK) { xr[XCOL(Kc + 8, el)] = w * sval * nn;  xi[XCOL(Kc + 8, el)] = 0.0; }
      }
      // rows beyond the window (the virtual sample u = -1 and the tail of the last chunk): zero
      if (d0 + PE > mid) {
        for (int q = tid; q < TS * 16 * nb; q += nt_thr) {
          const int row = q / (16 * nb), col = q - row * (16 * nb);
          const int d = d0 + (row >> 1);
          const int t = (row & 1) ? (mid + d) : (mid - d - 1);
          if (d > mid || t < 0) { Xre[row * ldx + col] = 0.0; Xim[row * ldx + col] = 0.0; }
        }
      }
      LS_STAMP(12);
      __syncthreads();
      LS_STAMP(1);
      const int pcs = (npairs - d0 < PE) ? (npairs - d0) : PE;   // sample pairs in this chunk
      const int ksl = (pcs + 1) >> 1;                             // k-steps (4 rows each) that hold samples
      if constexpr (UN > 0) {
        // Whole pairs first — a pair's three weights share the four LDS reads and the n-scaled operands of a k-step (the
        // f64 vector instructions that prepare operands do not run beside the f64 MFMAs here: dealt out as 63 single units
        // with their own scaling, the contraction was slower than the stacked one in spite of 30 % fewer MFMAs) — then the
        // single units.  Not software-pipelined, like the whole-pair loop below: every loop kind was tried with the operands
        // of k-step ks + 1 read ahead of the MFMAs of k-step ks, and no class gained (profiles/tw_pipeline/README.md).
        const int plane = TS * ldx_max;
        const int kn = (ksl < 8) ? ksl : 8;
#pragma unroll
        for (int gi = 0; gi < GA + GB; ++gi) {
          const int s0 = (gi < GA) ? 3 * gi : UA + 3 * (gi - GA);   // first slot of the group
          const int code = ucode[s0];
          if (code == 0xFFFF) continue;
          const int ca = 16 * ((code >> 8) & 15), cb = 16 * ((code >> 4) & 15);
          const bool k4 = (code & 3) == 1;
          int rb = lq * ldx;
          const int sw0 = lcol + (lq >> 1);
          // n_k of this lane's row 4 ks + lq: sample pair d = d0 + 2 ks + lq/2, odd rows t = mid + d, even rows t = mid - d - 1
          int nk = (lq & 1) ? d0 + (lq >> 1) : -d0 - (lq >> 1) - 1;
          asm volatile("" : "+v"(rb), "+v"(nk));   // (hoisted out of the chunk loop, these spill)
          if (PK && gi >= GA) {   // (constant once the group loop is unrolled: edge pairs sit in two-accumulator groups only)
            if (code & 0x1000) {   // an edge pair: its two units in the group's first two slots
              const int q = (gi >= GA) ? 3 * (gi - GA) : 0;
#pragma clang loop unroll(disable)
              for (int ks = 0; ks < kn; ++ks) {
                const int sw = (sw0 + 2 * ks) & 15;
                const double aR = Xre[rb + ca + sw], aI = Xre[rb + ca + sw + plane];
                const double bR = Xre[rb + cb + sw], bI = Xre[rb + cb + sw + plane];
                rb += 4 * ldx;
                twu_edge_k4(gb[q], gb[q + 1], aR, aI, bR, bI, (double)nk);
                nk += (lq & 1) ? 2 : -2;
              }
              continue;
            }
          }
#pragma clang loop unroll(disable)
          for (int ks = 0; ks < kn; ++ks) {
            const int sw = (sw0 + 2 * ks) & 15;
            const double aR = Xre[rb + ca + sw], aI = Xre[rb + ca + sw + plane];
            const double bR = Xre[rb + cb + sw], bI = Xre[rb + cb + sw + plane];
            rb += 4 * ldx;
            if (gi < GA) {
              const int q = (gi < GA) ? 3 * gi : 0;
              twu_pair_k3(ga[q], ga[q + 1], ga[q + 2], aR, aI, bR, bI, (double)nk);
            } else {
              const int q = (gi >= GA) ? 3 * (gi - GA) : 0;
              twu_pair_2acc(gb[q], gb[q + 1], gb[q + 2], aR, aI, bR, bI, (double)nk, k4);
            }
            nk += (lq & 1) ? 2 : -2;
          }
        }
#pragma unroll
        for (int sl = 0; sl < UN; ++sl) {
          if ((sl < UA) ? (sl < 3 * GA) : (sl - UA < 3 * GB)) continue;   // a slot of a whole pair
          const int code = ucode[sl];
          if (code == 0xFFFF) continue;
          const int ca = 16 * ((code >> 8) & 15), cb = 16 * ((code >> 4) & 15), up = (code >> 2) & 3;
          const bool k4 = (code & 3) == 1;
          int rb = lq * ldx;
          const int sw0 = lcol + (lq >> 1);
          int nk = (lq & 1) ? d0 + (lq >> 1) : -d0 - (lq >> 1) - 1;
          asm volatile("" : "+v"(rb), "+v"(nk));
          // the weight scales the operands (p >= 1: a by n_k, p = 2: b as well): one loop per weight, so that a unit pays
          // for the scalings it needs and for no selects.  P = 3: an edge unit with q = 1, b alone is scaled (q = 0 and the
          // corner run unscaled, as P = 0)
          auto run = [&](auto pc) {
            constexpr int P = decltype(pc)::value;
#pragma clang loop unroll(disable)
            for (int ks = 0; ks < kn; ++ks) {
              const int sw = (sw0 + 2 * ks) & 15;
              double aR = Xre[rb + ca + sw], aI = Xre[rb + ca + sw + plane];
              double bR = Xre[rb + cb + sw], bI = Xre[rb + cb + sw + plane];
              rb += 4 * ldx;
              if constexpr (P == 1 || P == 2) { aR *= (double)nk; aI *= (double)nk; }
              if constexpr (P >= 2) { bR *= (double)nk; bI *= (double)nk; }
              nk += (lq & 1) ? 2 : -2;
              if (sl < UA) {
                d4 (&g)[3] = ga[sl < UA ? sl : 0];
                g[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bR, g[0], 0, 0, 0);
                g[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, bI, g[1], 0, 0, 0);
                g[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR + aI, bI - bR, g[2], 0, 0, 0);
              } else {
                d4 (&g)[2] = gb[sl >= UA ? sl - UA : 0];
                g[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bR, g[0], 0, 0, 0);
                g[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bI, g[1], 0, 0, 0);
                g[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, bI, g[0], 0, 0, 0);
                if (k4) g[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(-aI, bR, g[1], 0, 0, 0);
              }
            }
          };
          if (up == 0) run(std::integral_constant<int, 0>{});
          else if (PK && (code & 0x1000)) run(std::integral_constant<int, PK ? 3 : 1>{});
          else if (up == 1) run(std::integral_constant<int, 1>{});
          else run(std::integral_constant<int, 2>{});
        }
      } else if constexpr (TW > 0) {
#pragma unroll
        for (int sl = 0; sl < TW; ++sl) {
          if (!glive[sl]) continue;
          const int ca = 16 * gI[sl], cb = 16 * gJ[sl];
          int rb = lq * ldx;
          const int sw0 = lcol + (lq >> 1);
          // n_k of this lane's row 4 ks + lq: sample pair d = d0 + 2 ks + lq/2, odd rows t = mid + d, even rows t = mid - d - 1
          int nk = (lq & 1) ? d0 + (lq >> 1) : -d0 - (lq >> 1) - 1;
          asm volatile("" : "+v"(rb), "+v"(nk));   // (hoisted out of the chunk loop, these spill)
          const int plane = TS * ldx_max;
          // (not software-pipelined: the registers allow it — no spill with the operands of the next k-step read ahead, moved
          // or in a loop of two k-steps — but it measured no faster, with the moves 3.5 % slower: the LDS round trip is not
          // exposed, the SIMD's other wave fills it; what the loop loses against the MFMA rate is the FP64 vector work of the
          // scalings, which shares the pipe.  profiles/tw_pipeline/README.md)
          int kn = (ksl < 8) ? ksl : 8;
          int ks = 0;
          if (split && sl == 1) {   // this wave's half of the chunk's k-steps
            if (wave & 1) { ks = 4; rb += 16 * ldx; nk += (lq & 1) ? 8 : -8; }
            else kn = (kn < 4) ? kn : 4;
          }
#pragma clang loop unroll(disable)
          for (; ks < kn; ++ks) {
            const int sw = (sw0 + 2 * ks) & 15;
            const double aR = Xre[rb + ca + sw], aI = Xre[rb + ca + sw + plane];
            const double bR = Xre[rb + cb + sw], bI = Xre[rb + cb + sw + plane];
            rb += 4 * ldx;
            tw_step(g[sl], aR, aI, bR, bI, (double)nk);
            nk += (lq & 1) ? 2 : -2;
          }
        }
      } else {
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
          if (!live[sl]) continue;
          const int ca = 16 * tP[sl], cb = 16 * tQ[sl];
          // operands of k-step ks+1 are requested before the MFMAs of k-step ks are issued (LDS latency hidden
          // behind the matrix pipe); row = 4 ks + lq, column swizzle (lcol + row/2) & 15
          int rb = lq * ldx;
          const int sw0 = lcol + (lq >> 1);
          asm volatile("" : "+v"(rb));   // keep the address arithmetic inside the loop (hoisted, it spills)
          const int plane = TS * ldx_max;
          if (ksl < 8) {   // last chunk of the window: only the k-steps that hold samples (the other rows are zero)
#pragma clang loop unroll(disable)
            for (int ks = 0; ks < ksl; ++ks) {
              const int sw = (sw0 + 2 * ks) & 15;
              const double aR = Xre[rb + ca + sw], aI = Xre[rb + ca + sw + plane];
              const double bR = Xre[rb + cb + sw], bI = Xre[rb + cb + sw + plane];
              rb += 4 * ldx;
              if (sl < NM3) {
                accR[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bR, accR[sl], 0, 0, 0);
                acc3[sl < NM3 ? sl : 0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, bI, acc3[sl < NM3 ? sl : 0], 0, 0, 0);
                accI[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR + aI, bI - bR, accI[sl], 0, 0, 0);
              } else {
                accR[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bR, accR[sl], 0, 0, 0);
                accI[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bI, accI[sl], 0, 0, 0);
                accR[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, bI, accR[sl], 0, 0, 0);
                accI[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(-aI, bR, accI[sl], 0, 0, 0);
              }
            }
            continue;
          }
          double aR, aI, bR, bI;
          {
            const int sw = sw0 & 15;
            aR = Xre[rb + ca + sw]; aI = Xre[rb + ca + sw + plane]; bR = Xre[rb + cb + sw]; bI = Xre[rb + cb + sw + plane];
          }
#pragma unroll
          for (int ks = 0; ks < 8; ++ks) {   // TS = 32 rows
            double naR = 0, naI = 0, nbR = 0, nbI = 0;
            if (ks < 7) {
              rb += 4 * ldx;
              const int sw = (sw0 + 2 * (ks + 1)) & 15;
              naR = Xre[rb + ca + sw]; naI = Xre[rb + ca + sw + plane]; nbR = Xre[rb + cb + sw]; nbI = Xre[rb + cb + sw + plane];
            }
            __builtin_amdgcn_sched_barrier(0);   // the requests above stay ahead of the MFMAs below
            if (sl < NM3) {   // three real products per complex one: P1 = aR bR, P2 = aI bI, P3 = (aR+aI)(bI-bR)
              accR[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bR, accR[sl], 0, 0, 0);
              acc3[sl < NM3 ? sl : 0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, bI, acc3[sl < NM3 ? sl : 0], 0, 0, 0);
              accI[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR + aI, bI - bR, accI[sl], 0, 0, 0);
            } else {
              accR[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bR, accR[sl], 0, 0, 0);
              accI[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bI, accI[sl], 0, 0, 0);
              accR[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, bI, accR[sl], 0, 0, 0);
              accI[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(-aI, bR, accI[sl], 0, 0, 0);
            }
            aR = naR; aI = naI; bR = nbR; bI = nbI;
          }
        }
      }
      __syncthreads();
      LS_STAMP(2);
    }
    if constexpr (TW == 0 && NM3 > 0) {   // Re = P1 + P2,  Im = aR bI - aI bR = P3 + P1 - P2
#pragma unroll
      for (int sl = 0; sl < NM3; ++sl) {
        const d4 p1 = accR[sl], p2 = acc3[sl];
        accR[sl] = p1 + p2;
        accI[sl] = accI[sl] + (p1 - p2);
      }
    }
    if constexpr (LDS_XCH) {
      // The G_p tiles change hands in LDS (eaqhm_ls_tilexch.h): region U is dead between the last chunk's closing barrier and
      // the barrier in front of the factorisation.  Y = [X_E | n X_E | s] with X = [X_E | s], so entry (R, C) of Y^H Y is
      // G_p[a][b]: a = R (amplitude row), R - Kc (slope row) or Kc (signal row), likewise b for C, p = the number of slope
      // indices among R and C.  Every G_p is Hermitian (n is real): entries above the tile diagonal of G_p are conjugates of
      // computed ones.  A round: stores of its planes, barrier, the gather of the entries stored in it, and a barrier before
      // the next round's stores; the last round closes on the barrier in front of the factorisation (dflag, which thread 0
      // zeroes ahead of that barrier, lies behind the exchange area).  PPR planes per round: all three for T <= 4 (class of
      // <= 8 tile rows), {0, 1} then {2} for T = 5 (9 and 10 tile rows).
      constexpr int PPR = NS == 5 ? 3 : 2, NR = NS == 5 ? 1 : 2;
      static_assert(PPR == tx_planes_per_round(NS == 5 ? 4 : 5) && NR == tx_rounds(NS == 5 ? 4 : 5), "rounds of eaqhm_ls_tilexch.h");
      typedef __attribute__((address_space(3))) char* xch_base_t;
      typedef int xch_i4 __attribute__((ext_vector_type(4)));
      typedef double xch_d2 __attribute__((ext_vector_type(2)));
      typedef __attribute__((address_space(3))) xch_d2* xch_cell_t;
      xch_base_t Xb = (xch_base_t)(char*)U;
      // The gather's index table (eaqhm_ls_gather.h), one entry per row / column index of the frame, and the zero that
      // padding positions and empty slots read: in `win` and at the start of `sig`, which nothing reads once the last chunk is
      // built; written beside the first round's stores, published by the barrier behind them.
      const unsigned tabB = (unsigned)tx_table_byte(uni(A.Kcmax)), zcB = (unsigned)tx_zcell_byte(uni(A.Kcmax));
      const __attribute__((address_space(3))) xch_i4* gtab = (const __attribute__((address_space(3))) xch_i4*)(Xb + tabB);
      if (tid < 16 * nt) {
        const GatherEntry e = gather_entry(tid, Kc, npair, T, false);
        *(__attribute__((address_space(3))) xch_i4*)(Xb + tabB + 32 * tid) = (xch_i4){e.lo, e.hi, e.trow, e.tcol};
      }
      if (tid == TL_THREADS - 1) *(xch_cell_t)(Xb + zcB) = (xch_d2){0.0, 0.0};
      const unsigned span = (unsigned)(PPR * TX_TILE_BYTES * npair);   // bytes of a round's planes
      static_assert(NR == 1 || (NR == 2 && PPR == 2), "a round after the first holds G_2 alone");
      unsigned gup[NS];
#pragma unroll
      for (int rd = 0; rd < NR; ++rd) {
        // ---- stores: entry (i, j) = (lq + 4 r, lcol) of this lane, its 16-byte cell XOR the row (tx_swizzle).  The second
        // halves of a split pair (T = 4) wait for the first halves and are added in place, first half + second half.
#pragma unroll
        for (int sl = 0; sl < TWA; ++sl) {
          if (!glive[sl]) continue;
          const bool second = split && sl == 1 && (wave & 1);
          if (second) continue;
#pragma unroll
          for (int p = 0; p < 3; ++p) {
            if (p / PPR != rd) continue;
            const d4 p1 = g[sl][3 * p], p2 = g[sl][3 * p + 1];
            const d4 re = p1 + p2, im = g[sl][3 * p + 2] + (p1 - p2);
            const unsigned tb = (unsigned)(TX_TILE_BYTES * ((p % PPR) * npair + gx[sl]));
#pragma unroll
            for (int r = 0; r < 4; ++r)
              *(xch_cell_t)(Xb + tb + tx_swizzle((unsigned)(256 * (lq + 4 * r) + 16 * lcol))) = (xch_d2){re[r], im[r]};
          }
        }
        __syncthreads();
        if (NS == 5 && split) {
          if (glive[TWA - 1] && (wave & 1)) {   // (the second halves live in the last slot of waves 1 and 3)
#pragma unroll
            for (int p = 0; p < 3; ++p) {
              const d4 p1 = g[TWA - 1][3 * p], p2 = g[TWA - 1][3 * p + 1];
              const d4 re = p1 + p2, im = g[TWA - 1][3 * p + 2] + (p1 - p2);
              const unsigned tb = (unsigned)(TX_TILE_BYTES * (p * npair + gx[TWA - 1]));
              xch_d2 c1[4];
#pragma unroll
              for (int r = 0; r < 4; ++r) c1[r] = *(xch_cell_t)(Xb + tb + tx_swizzle((unsigned)(256 * (lq + 4 * r) + 16 * lcol)));
#pragma unroll
              for (int r = 0; r < 4; ++r)
                *(xch_cell_t)(Xb + tb + tx_swizzle((unsigned)(256 * (lq + 4 * r) + 16 * lcol))) = (xch_d2){c1[r].x + re[r], c1[r].y + im[r]};
            }
          }
          __syncthreads();
        }
        // ---- gather.  Every slot, empty ones too: nothing of accR / accI lives through the contraction.  The first round
        // loads every value — an entry of a later round and padding read the zero cell — straight into the accumulator
        // registers, all requests ahead of the first use.  The second round (G_2 alone: entries whose row and column are
        // both slope indices) is skipped by the slots that cannot have one — wave-uniform, from where Kc and 2 Kc fall in
        // the tile's rows and columns —, the others look their offsets up again (kept from the first round they cost
        // the 7-slot budget its registers: vector scratch, and 2.8 k cycles in the back substitution) and take the value
        // where the entry's plane is in the round.  Only the sign of the imaginary part is left to fix afterwards: one
        // word per slot holds the four `up` bits.
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
          if (rd > 0) {
            const int r0 = 16 * tP[sl], c0 = 16 * tQ[sl];
            if (!(r0 + 15 >= Kc && r0 < 2 * Kc && c0 + 15 >= Kc && c0 < 2 * Kc)) continue;
          }
          unsigned off[4];
          {
            // column entry once per slot (an empty slot: index 16 nt - 1, which is padding in every frame: 2 Kc + 1 is odd)
            const int cx = live[sl] ? 16 * tQ[sl] + lcol : 16 * nt - 1;
            const __attribute__((address_space(3))) xch_i4* rt = gtab + 2 * (16 * tP[sl] + lq);
            xch_i4 c0 = gtab[2 * cx], r0[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) r0[r] = rt[8 * r];
            // (the entries whole, ahead of their use: left alone the compiler sinks each word's read into a branch on `up`
            // and waits for it there)
            asm volatile("" : "+v"(c0.x), "+v"(c0.y), "+v"(c0.w));
#pragma unroll
            for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(r0[r].x), "+v"(r0[r].y), "+v"(r0[r].z));
            unsigned ups = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int dt = r0[r].z - c0.w;   // < 0: above the tile diagonal, the conjugate of a stored entry (eaqhm_ls_gather.h)
              const unsigned o = (unsigned)((dt < 0 ? r0[r].y : r0[r].x) + (dt < 0 ? c0.x : c0.y));
              off[r] = o < (unsigned)GI_ZCELL ? o : (unsigned)GI_ZCELL;
              ups = (ups >> 1) | ((unsigned)dt & 0x80000000u);
            }
            if (rd == 0) gup[sl] = ups;
          }
          if (rd == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {   // (one round: off < span for every entry but padding)
              const xch_d2 v = *(xch_cell_t)(Xb + (off[r] < span ? tx_swizzle(off[r]) : zcB));
              accR[sl][r] = v.x; accI[sl][r] = v.y;
            }
          } else {
            bool in[4];
            xch_d2 v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              off[r] -= (unsigned)rd * span;   // (padding: GI_ZCELL lies more than a span behind the last plane)
              in[r] = off[r] < span;
              v[r] = *(xch_cell_t)(Xb + (in[r] ? tx_swizzle(off[r]) : zcB));
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              accR[sl][r] = in[r] ? v[r].x : accR[sl][r];
              accI[sl][r] = in[r] ? v[r].y : accI[sl][r];
            }
          }
        }
        if (rd + 1 < NR) __syncthreads();   // the round's tiles are read: the next round's stores may overwrite them
      }
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {   // -im where `up`: the sign bit
          const double vi = accI[sl][r];
          accI[sl][r] = __hiloint2double(__double2hiint(vi) ^ (int)((gup[sl] << (3 - r)) & 0x80000000u), __double2loint(vi));
        }
      }
      // the exchange on a slot of its own (9), so that slot 2 is the k-step loops and the chunk's closing barrier alone; with
      // the diag_D diagnostics on, slot 9 is theirs and the exchange stays in slot 2
      LS_STAMP(uni((int)A.debug_diag) ? 2 : 9);
    }
    if constexpr (G3 && !LDS_XCH) {
      // The unit tables (UN > 0): the G_p tiles go through the workgroup's scratch area (the bridged track rows are dead now; <= 3 * 21 tiles of
      // 16 x 16 complex values, see ls_tile_scratch_stride), then every wave gathers its system tiles.  Y = [X_E | n X_E | s]
      // with X = [X_E | s], so entry (R, C) of Y^H Y is G_p[a][b]: a = R (amplitude row), R - Kc (slope row) or Kc
      // (signal row), likewise b for C, p = the number of slope indices among R and C.  Every G_p is Hermitian (n is
      // real): entries above the tile diagonal of G_p are conjugates of computed ones.
      double* Gs = Qs;
      // The gather's index table (eaqhm_ls_gather.h), one entry per row / column index of the frame, and the zero that
      // padding positions and empty slots read: written beside the tile stores, published by the barrier behind them.
      // The table lies at the start of region U: the basis chunk is done with (the chunk's closing barrier), and nothing
      // is written there again before the barrier that follows the gather.
      int4* gtab = (int4*)U;
      if (tid < 16 * nt) {
        const GatherEntry e = gather_entry(tid, Kc, npair, T, PK);
        gtab[2 * tid] = make_int4(e.lo, e.hi, e.trow, e.tcol);
        if constexpr (PK) gtab[2 * tid + 1] = make_int4(e.mask, e.val, 0, 0);
      }
      if (tid == TL_THREADS - 1) *(double2*)((char*)Gs + GI_ZCELL) = make_double2(0.0, 0.0);
      if constexpr (UN > 0) {
        // a unit's tile: (Re, Im) for K3 and K4, (Re, RI) for H — the gather below takes Im = RI - RI^T there
#pragma unroll
        for (int sl = 0; sl < UN; ++sl) {
          const int code = ucode[sl];
          if (code == 0xFFFF) continue;
          const int I = (code >> 8) & 15, J = (code >> 4) & 15, up = (code >> 2) & 3;   // (edge units: plane q, the corner: plane 0)
          d4 re, im;
          if (sl < UA) {
            const d4 p1 = ga[sl < UA ? sl : 0][0], p2 = ga[sl < UA ? sl : 0][1];
            re = p1 + p2; im = ga[sl < UA ? sl : 0][2] + (p1 - p2);
          } else {
            re = gb[sl >= UA ? sl - UA : 0][0]; im = gb[sl >= UA ? sl - UA : 0][1];
          }
          double* gt = Gs + (size_t)(up * npair + I * (I + 1) / 2 + J) * 512;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = 2 * (16 * (lq + 4 * r) + lcol);
            gt[o] = re[r]; gt[o + 1] = im[r];
          }
        }
      }
      __syncthreads();
      if constexpr (UN > 0) {
        // H units hold (Re, RI): Im = RI - RI^T in place, so that the gather reads every tile alike and needs no second
        // value per entry (packed tables: the corner has plane 0 only).  A thread takes both entries of a transposed pair
        // (i, j), i <= j: 136 pairs per diagonal tile, rows r and 15 - r of the triangle side by side (17 entries);
        // T = TWU_TT[TB] here.  Every load ahead of the first store and no branch but in the last round: one round trip
        // through the L2, not one per tile.
        constexpr int TT = TWU_TT[TB], HN = (PK ? 3 * (TT - 1) + 1 : 3 * TT) * 136, HF = HN / TL_THREADS, HT = HF + (HN % TL_THREADS ? 1 : 0);
        double ha[HT], hb[HT];
        int hoa[HT], hob[HT];
#pragma unroll
        for (int k = 0; k < HT; ++k) {
          const int q = tid + k * TL_THREADS, qc = (q < HN) ? q : 0;
          const int t = qc / 136, e = qc - 136 * t, r = e / 17, c = e - 17 * r;
          const int i = (c < 16 - r) ? r : 15 - r, j = (c < 16 - r) ? r + c : c - 1;
          const int TD = PK ? TT - 1 : TT, pl = (t < 3 * TD) ? t / TD : 0, I = (t < 3 * TD) ? t - pl * TD : TT - 1;   // (packed: the corner last)
          const int tile = (pl * npair + I * (I + 1) / 2 + I) * 512;
          hoa[k] = tile + 2 * (16 * i + j) + 1; hob[k] = tile + 2 * (16 * j + i) + 1;
          ha[k] = Gs[hoa[k]]; hb[k] = Gs[hob[k]];
        }
#pragma unroll
        for (int k = 0; k < HT; ++k) {
          if (k < HF || tid + k * TL_THREADS < HN) {
            Gs[hoa[k]] = ha[k] - hb[k];
            Gs[hob[k]] = hb[k] - ha[k];   // (i = j: the same place, the same zero)
          }
        }
        __syncthreads();
      }
      // Every slot, empty ones too: nothing of accR / accI lives through the contraction.  The loads of the gather are
      // issued unconditionally and consumed afterwards: the values come out of the L2, and a load inside a branch of its own
      // is waited for before the next address is even computed — one exposed round trip per value, 4 NS of them per frame
      // (22 k to 52 k cycles, 6-7 % of a frame).
      // One batch for every budget: a value is loaded into its accumulator registers — padding reads the zero cell, so
      // nothing is selected afterwards — and only the sign of the imaginary part is left to fix: one word per slot holds
      // the four `up` bits (bit 31 - 3 + r for row r).  The address is the wave-uniform Gs plus a 32-bit byte offset.
      typedef const __attribute__((address_space(1))) char* gather_base_t;
      gather_base_t Gb = (gather_base_t)(const char*)Gs;
      unsigned gup[NS];
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) {
        // column entry once per slot (an empty slot: index 16 nt - 1, which is padding in every frame: 2 Kc + 1 is odd)
        const int cx = live[sl] ? 16 * tQ[sl] + lcol : 16 * nt - 1;
        const int4* rt = gtab + 2 * (16 * tP[sl] + lq);
        int4 c0 = gtab[2 * cx], c1 = make_int4(0, 0, 0, 0), r0[4], r1[4];
        if constexpr (PK) c1 = gtab[2 * cx + 1];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          r0[r] = rt[8 * r];
          if constexpr (PK) r1[r] = rt[8 * r + 1];
        }
        // (the entries whole, ahead of their use: left alone the compiler sinks each word's read into a branch on `up` and
        // waits for it there)
        asm volatile("" : "+v"(c0.x), "+v"(c0.y), "+v"(c0.w));
        if constexpr (PK) asm volatile("" : "+v"(c1.x), "+v"(c1.y));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          asm volatile("" : "+v"(r0[r].x), "+v"(r0[r].y), "+v"(r0[r].z));
          if constexpr (PK) asm volatile("" : "+v"(r1[r].x), "+v"(r1[r].y));
        }
        unsigned ups = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int dt = r0[r].z - c0.w;   // < 0: above the tile diagonal, the conjugate of a stored entry (eaqhm_ls_gather.h)
          unsigned off = (unsigned)((dt < 0 ? r0[r].y : r0[r].x) + (dt < 0 ? c0.x : c0.y));
          if constexpr (PK) off += (unsigned)((dt < 0 ? c1.x : r1[r].x) & (dt < 0 ? r1[r].y : c1.y));
          off = off < (unsigned)GI_ZCELL ? off : (unsigned)GI_ZCELL;
          ups = (ups >> 1) | ((unsigned)dt & 0x80000000u);
          typedef double gather_d2 __attribute__((ext_vector_type(2)));
          const gather_d2 v = *(const __attribute__((address_space(1))) gather_d2*)(Gb + off);
          accR[sl][r] = v.x; accI[sl][r] = v.y;
        }
        gup[sl] = ups;
      }
      __builtin_amdgcn_sched_barrier(0);   // every request ahead of the first use: one round trip through the L2 per frame
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {   // -im where `up`: the sign bit
          const double vi = accI[sl][r];
          accI[sl][r] = __hiloint2double(__double2hiint(vi) ^ (int)((gup[sl] << (3 - r)) & 0x80000000u), __double2loint(vi));
        }
      }
      // the gather on a slot of its own (9), so that slot 2 is the k-step loops and the chunk's closing barrier alone; with
      // the diag_D diagnostics on, slot 9 is theirs and the gather stays in slot 2
      LS_STAMP(uni((int)A.debug_diag) ? 2 : 9);
    }

    {
      // ---- padding positions of the last tile row/column (beyond the signal) get an identity row/column
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) {
        if (!live[sl] || tP[sl] != nt - 1) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = lq + 4 * r, col = lcol;
          const bool pad = (row > is) || (tQ[sl] == nt - 1 && col > is);
          if (pad) {
            accR[sl][r] = (tQ[sl] == nt - 1 && row == col) ? 1.0 : 0.0;
            accI[sl][r] = 0.0;
          }
        }
      }
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) {   // original diagonal entries, for the collapsed-pivot check of diag_coop
        if (!live[sl] || tP[sl] != tQ[sl]) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (lq + 4 * r == lcol) dorig[16 * tP[sl] + lcol] = accR[sl][r];
      }
      // Right-looking tile Cholesky with look-ahead.  Stage jb: the trailing update with panel jb-1 — the diagonal tile
      // (jb, jb) first, whose owner then factorises and inverts it on its own (diag_wave: one wave, matrix cores, no
      // workgroup barrier) while the other waves are still in their updates — barrier — panel jb — barrier.
      double* post = Dc;                 // what diag_D posts for diag_Z (Dc and Zc are contiguous: 1088 doubles)
      double* dumpD = Dc + DGP_DOUBLES;  // [128] dump slots of diag_D
      double* zs = dumpD + 128;          // [256] row exchange, dump slots and row factors of diag_Z
      int* dflag = (int*)(zs + 256);     // step counter of the diagonal pipeline
      if (tid == 0) *dflag = 0;          // (region U held the last basis chunk until the barrier that ended the Gramian)
      __syncthreads();
#define TRAILING_UPDATE(sl)                                                                         \
  {                                                                                                 \
    const double* ar = PanR + tP[sl] * TL_TILE;                                                     \
    const double* ai = PanI + tP[sl] * TL_TILE;                                                     \
    const double* br = PanR + tQ[sl] * TL_TILE;                                                     \
    const double* bi = PanI + tQ[sl] * TL_TILE;                                                     \
    /* T -= L_P L_Q^H, three real products: P1 = re re', P2 = im im', P3 = (re+im)(im'-re');   */   \
    /* Re -= P1 + P2,  Im += P3 + P1 - P2  (P3 accumulates straight into the imaginary part)   */   \
    d4 p1 = (d4){0, 0, 0, 0}, p2 = (d4){0, 0, 0, 0};                                                \
    _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) {                                              \
      const int o = (4 * ks + lq) * TL_LD + lcol;                                                   \
      const double aR = ar[o], aI = ai[o], lR = br[o], lI = bi[o];                                  \
      p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, lR, p1, 0, 0, 0);                               \
      p2 = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, lI, p2, 0, 0, 0);                               \
      accI[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(aR + aI, lI - lR, accI[sl], 0, 0, 0);         \
    }                                                                                               \
    accR[sl] = accR[sl] - (p1 + p2);                                                                \
    accI[sl] = accI[sl] + (p1 - p2);                                                                \
  }
      for (int jb = 0; jb < nt; ++jb) {
        d4 Rt = (d4){0, 0, 0, 0}, It = (d4){0, 0, 0, 0};
        bool mine = false;
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
          if (!live[sl] || tP[sl] != jb || tQ[sl] != jb) continue;
          if (jb > 0) TRAILING_UPDATE(sl)
          Rt = accR[sl]; It = accI[sl];
          mine = true;
        }
        // real unknowns: every position but, in the last tile, the signal column `is` and the padding behind it
        if (mine) {
          unsigned long long td0 = 0;
          unsigned long long* tlast = (unsigned long long*)(dflag + 2);   // (diagnostics: end of the previous diag_D)
          const bool tdiag = dbg && uni(A.debug_diag);
          if (tdiag) td0 = __builtin_amdgcn_s_memtime();
          diag_D(Rt, It, post, nullptr, dflag, 16 * jb, dumpD, LdR, LdI, jb == nt - 1);
          if (tdiag && lane == 0) {   // slots 9 / 11 / 13 / 14: cycles inside diag_D, from one diag_D to the next, counts
            const unsigned long long td1 = __builtin_amdgcn_s_memtime();
            atomicAdd(dbg + 9, td1 - td0);
            if (jb > 0) { atomicAdd(dbg + 11, td0 - *tlast); atomicAdd(dbg + 14, 1ull); }
            atomicAdd(dbg + 13, 1ull);
            *tlast = td1;
          }
        }
        LS_STAMP(10);
        if (jb > 0) {
#pragma unroll
          for (int sl = 0; sl < NS; ++sl) {
            if (!live[sl] || tQ[sl] < jb || (tP[sl] == jb && tQ[sl] == jb)) continue;
            TRAILING_UPDATE(sl)
          }
        }
        LS_STAMP(8);
        // Stage 0 has no trailing update: every wave but the owner of the first diagonal tile and its helper is about to
        // wait at barrier A.  The first of them fetches the next frame's header meanwhile (TlHead).
        // Its slot list goes to the buffer this frame's is not in.
        if (NEXT_HEAD && jb == 0) {
          int pfw = 0;
          while (pfw == DIAG_OWNER(0, nt) || pfw == (int)TL_HELP[nt][0]) ++pfw;
          if (wave == pfw) fetch_next_header(A, hd, C, uni(hd->buf) ^ 1, lane);
        }
        // The helper wave builds the inverse (eaqhm_ls_tilemap.h) — AFTER its own trailing tiles: diag_D's posts wait for
        // it in LDS and it runs through them without the owner's pace, so its tiles are not what the stage ends on.
        if (!mine && wave == (int)TL_HELP[nt][jb])
          diag_Z(post, dflag, 16 * jb, zs, WtR + jb * TL_TILE, WtI + jb * TL_TILE, dorig + 16 * jb,
                 (jb == nt - 1) ? is : 16, uni(A.fault));
        __syncthreads();  // (A) inverse of the diagonal tile published; every read of panel jb-1 done
        LS_STAMP(6);
        // ---- panel tiles (P > jb, Q == jb): X = T W^H, published as Pan[P][k][row]
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
          if (!live[sl] || tQ[sl] != jb || tP[sl] == jb) continue;
          double* tr = PanR + tP[sl] * TL_TILE;   // the tile's own panel slot doubles as transposition buffer
          double* ti = PanI + tP[sl] * TL_TILE;
#pragma unroll
          for (int r = 0; r < 4; ++r) {  // T[row = lq+4r][col = lcol] -> tmp[k = col][i = row]
            tr[lcol * TL_LD + lq + 4 * r] = accR[sl][r];
            ti[lcol * TL_LD + lq + 4 * r] = accI[sl][r];
          }
          __builtin_amdgcn_wave_barrier();
          // X = T W^H with three real products per complex one: P1 = re re, P2 = im im, P3 = (re+im)(re'+im')
          d4 p1 = (d4){0, 0, 0, 0}, p2 = (d4){0, 0, 0, 0}, p3 = (d4){0, 0, 0, 0};
          const double* wr = WtR + jb * TL_TILE;
          const double* wi = WtI + jb * TL_TILE;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const int o = (4 * ks + lq) * TL_LD + lcol;
            const double aR = tr[o], aI = ti[o], bR = wr[o], bI = wi[o];
            p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aR, bR, p1, 0, 0, 0);
            p2 = __builtin_amdgcn_mfma_f64_16x16x4f64(aI, bI, p2, 0, 0, 0);
            p3 = __builtin_amdgcn_mfma_f64_16x16x4f64(aR + aI, bR + bI, p3, 0, 0, 0);
          }
          const d4 xr = p1 - p2, xi = p3 - (p1 + p2);
          accR[sl] = xr; accI[sl] = xi;  // the finished L tile stays here for the back substitution
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            tr[lcol * TL_LD + lq + 4 * r] = xr[r];
            ti[lcol * TL_LD + lq + 4 * r] = xi[r];
          }
        }
        LS_STAMP(7);
        __syncthreads();  // (C) panel jb published
      }
#undef TRAILING_UPDATE
      __syncthreads();  // end of factorisation
      LS_STAMP(3);

      // ============ back substitution  L^H x = y,  y = conj(row `is` of the last tile row) ============
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) {
        if (!live[sl] || tP[sl] != nt - 1 || tQ[sl] == nt - 1) continue;
        if (lq == (is & 3)) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (r == (is >> 2)) {
              zv[2 * (16 * tQ[sl] + lcol)] = accR[sl][r];
              zv[2 * (16 * tQ[sl] + lcol) + 1] = -accI[sl][r];
            }
        }
      }
      if (tid < 16) {
        const bool ok = tid < is;
        zv[2 * (16 * (nt - 1) + tid)] = ok ? LdR[is * TL_LD + tid] : 0.0;
        zv[2 * (16 * (nt - 1) + tid) + 1] = ok ? -LdI[is * TL_LD + tid] : 0.0;
      }
      for (int q = tid; q < 4 * Kc; q += nt_thr) xs[q] = 0.0;
      __syncthreads();  // y gathered
      for (int P = nt - 1; P >= 0; --P) {
        if (tid < 256) {  // x_P = W_PP^H z_P : thread (i, k) takes one term of row i, 16-lane shuffle reduction
          const int i = tid >> 4, k = tid & 15;
          double xr = 0, xi = 0;
          if (k >= i) {   // W^H is upper triangular
            const double wr = WtR[P * TL_TILE + i * TL_LD + k], wi = WtI[P * TL_TILE + i * TL_LD + k];
            const double zr = zv[2 * (16 * P + k)], zi = zv[2 * (16 * P + k) + 1];
            xr = wr * zr - wi * zi;
            xi = wr * zi + wi * zr;
          }
          xr = sum16_first(xr); xi = sum16_first(xi);   // (the xor butterfly's additions, by row shifts)
          if (k == 0) {
            xv[2 * i] = xr; xv[2 * i + 1] = xi;
            const int q = 16 * P + i;   // natural order: amplitudes then slopes
            if (q < 2 * Kc) { xs[2 * q] = xr; xs[2 * q + 1] = xi; }
          }
        }
        __syncthreads();
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
          if (!live[sl] || tP[sl] != P || tQ[sl] == P) continue;
          double sr = 0, si = 0;  // sum_i conj(L[i][j]) x[i] over this lane's rows i = lq + 4r
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double xr = xv[2 * (lq + 4 * r)], xi = xv[2 * (lq + 4 * r) + 1];
            const double lr = accR[sl][r], li = accI[sl][r];
            sr += lr * xr + li * xi;
            si += lr * xi - li * xr;
          }
          sr = sum4rows_first(sr); si = sum4rows_first(si);   // ((s0 + s1) + (s2 + s3)) over the four row groups
          if (lq == 0) {
            zv[2 * (16 * tQ[sl] + lcol)] -= sr;
            zv[2 * (16 * tQ[sl] + lcol) + 1] -= si;
          }
        }
        __syncthreads();
      }
      LS_STAMP(4);
    }

    // REC_ROW: the record row is put together where the chunk masks of the slot set-up lie, if it fits: dead tile storage
    // now, and the next frame writes there only after its first barrier, so that no barrier is needed behind the row's
    // way out (nothing else that write_record reads after its last barrier is written by the next frame's head).
    if (REC_ROW && 3 * uni(A.Kmax) + 1 <= TL_NSLOT * CI_NCH)
      write_record<true>(A, xs, sh, mycols, f, n, inst, c, f0, seeds, hd->fmc, (double*)masks);
    else
      write_record(A, xs, sh, mycols, f, n, inst, c, f0, seeds);
    LS_STAMP(5);
    if (dbg && tid == 0) hd->t_last = t_prev;
  }
}

// Frames bucketed by the number of tile rows of their system (see LsArgs::cls).
__device__ inline int frame_class(int n) {
  const int nt = (2 * (2 * n + 1) + 1 + 15) >> 4;
  return nt <= 8 ? 0 : nt == 9 ? 1 : nt == 10 ? 2 : nt == 11 ? 3 : nt == 12 ? 4 : nt <= TL_NTMAX ? 5 : LS_BIG_CLASS;
}
extern "C" __global__ void __launch_bounds__(256) eaqhm_ls_classify_kernel(LsArgs A) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
  int cl = (f < A.n_frames) ? frame_class((A.mode == 0) ? A.frame_K[f] : A.ncol[f]) : -1;
  if (f < A.n_frames) {   // the frame's window [c - wl, c + wl] inside the signal and (mode 1, with the sample before it) inside the resident tracks
    if (!frame_window_ok(A, A.frame_c[f], A.frame_wl[f])) { cl = -1; atomicAdd(A.fault + 2, 1); }   // dropped: its record row is not written
  }
  if (A.mode == 1 && cl >= 0) {   // chunks of the zero counts this frame's window (and the sample before it) touches
    const long long c = A.frame_c[f], wl = A.frame_wl[f];
    const long long lo = (c - wl - 1 > 0) ? (c - wl - 1) : 0;
    for (long long ch = lo >> 10; ch <= ((c + wl) >> 10); ++ch) A.zflag[ch] = 1;
  }
  for (int c = 0; c < LS_NCLS; ++c) {   // one atomic per wave and class, positions from the ballot
    const unsigned long long m = __ballot(cl == c);
    if (m == 0ull) continue;
    int base = 0;
    if (lane == __ffsll((long long)m) - 1) base = atomicAdd(A.cls + c, __popcll(m));
    base = __shfl(base, __ffsll((long long)m) - 1);
    if (cl == c) A.cls[16 + (size_t)c * A.n_frames + base + __popcll(m & ((1ull << lane) - 1ull))] = f;
  }
}

// Zero counts of every frequency track, in chunks of 1024 samples (LsArgs::zloc / ztot): a frame then knows with two
// look-ups per slot whether its window needs bridging, instead of scanning n windows of N samples.
// fm / zloc: biased by the first resident sample t_lo (LsArgs), rows of Lt samples; samples outside [t_lo, t_lo + Lt) are
// not resident (no frame window of this launch reaches them) and count as nonzero.
// Grid: x = the 1024-sample chunks that overlap the resident window (first one: ch0), y = slots.
extern "C" __global__ void __launch_bounds__(256) eaqhm_ls_zero_prefix_kernel(const double* __restrict__ fm, long long Lt,
                                                                              long long t_lo, int ch0, int zchunks,
                                                                              const unsigned char* __restrict__ zflag,
                                                                              unsigned short* __restrict__ zloc,
                                                                              int* __restrict__ ztot) {
  __shared__ int wsum[4];
  const int k = blockIdx.y, ch = ch0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!zflag[ch]) return;   // no frame of this launch (this rank) looks here
  const long long base = (long long)ch << 10;
  int run = 0;
  for (int p = 0; p < 4; ++p) {
    const long long t = base + 256 * p + tid;
    const bool in = t >= t_lo && t < t_lo + Lt;
    const bool z = in && (fm[(size_t)k * Lt + t] == 0.0);
    const unsigned long long m = __ballot(z);
    const int incl = __popcll(m & ((lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1ull)));
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int v = wsum[w]; tot += v; if (w < wave) off += v; }
    if (in) zloc[(size_t)k * Lt + t] = (unsigned short)(run + off + incl);
    run += tot;
    __syncthreads();
  }
  if (tid == 0) ztot[(size_t)k * zchunks + ch] = run;
}

// One persistent launch for every frame size: each workgroup works through the size classes, largest first, with
// the register budget (tiles per wave) of the class.
// A frame of class C per turn.  Where the previous frame of the class left the next one's header (TlHead; mode 1 only), the
// item comes from there; otherwise — a workgroup's first frame, the first one of a class — from the cursor, as the header's
// was.  Every draw is used exactly once, and a workgroup draws one item past the end of each class, either way.
extern "C" __global__ void __launch_bounds__(TL_THREADS) eaqhm_ls_tile_kernel(LsArgs A, int TS, int ldx_max) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int nxt;
  TlHead* hd = (TlHead*)(lds + tl_head_offset());   // (mode 0: a0_frame lays the LDS out its own way, no header)
  if (threadIdx.x == 0 && A.mode != 0) { hd->cls = -1; hd->t_last = 0ull; hd->seeds = (A.any_seed && *A.any_seed != 0) ? 1 : 0; }
  __syncthreads();
#define TW_UNITS(TB) 0, TWU_UA, TWU_UB, TB   /* template arguments TW, UA, UB, TB of a class that contracts units by table TB */
#define RUN_CLASS(NSV, TWV, C)                                                             \
  for (;;) {                                                                             \
    if (A.mode != 0 && hd->cls == C) {                                                   \
      if (hd->f < 0) break;                                                              \
      tile_frame<NSV, TWV>(A, TS, ldx_max, lds, -1);                                     \
      continue;                                                                          \
    }                                                                                    \
    if (threadIdx.x == 0) { nxt = atomicAdd(A.cls + 8 + C, 1); if (A.mode != 0) hd->buf = 1; }   \
    __syncthreads();                                                                     \
    const int item = nxt;                                                                \
    __syncthreads();                                                                     \
    if (item >= A.cls[C]) break;                                                         \
    if (A.mode == 0) a0_frame<A0_NS, A0_M, 2>(A, lds, A.cls[16 + (size_t)C * A.n_frames + item], TZ_TB, TZ_NCH, 520, 64 * CI_NCH);                          \
    else tile_frame<NSV, TWV>(A, TS, ldx_max, lds, A.cls[16 + (size_t)C * A.n_frames + item]);          \
  }
  RUN_CLASS(12, 0, 5)   // 91 tiles, T = 7: stacked
  RUN_CLASS(10, TW_UNITS(TWU_TB_12), 4)   // 78 tiles, T = 6: 63 units of the three-weight Gramian (eaqhm_ls_twunits.h)
  RUN_CLASS(9, TW_UNITS(TWU_TB_11), 3)    // 66 tiles, T = 6, last tile column packed: 45 units + 10 edge units + the corner
  RUN_CLASS(7, 2, 2)    // 55 tiles, T = 5: 15 basis pairs
  RUN_CLASS(6, 2, 1)    // 45 tiles, T = 5
  RUN_CLASS(5, 2, 0)    // <= 36 tiles, T <= 4: <= 10 basis pairs
#undef RUN_CLASS
#undef TW_UNITS
}

bool ls_tile_applicable(int Kcmax, int Nmax) { return tl_applicable(Kcmax, Nmax); }   // (eaqhm_ls_tilelds.h)

size_t ls_tile_scratch_stride(int nmax, int Nmax) {
  const size_t Npad = (size_t)((Nmax + 63) >> 6) << 6;
  // three-weight G_p tiles of the unit tables (T = 6, 11 and 12 tile rows; T <= 5 exchanges them in LDS) and the gather's zero
  // cell behind them (GI_ZCELL)
  const size_t bridged = 2 * Npad * nmax, gram = (size_t)3 * 21 * 512 + 2;
  return ((bridged > gram ? bridged : gram) + 15) & ~(size_t)15;
}

// Frames into their size classes, and (adaptations >= 1) the zero counts of the tracks that the slot set-up of both
// batched kernels looks up.  A.cls (zeroed header) / A.zflag (zeroed) / A.zloc / A.ztot are set by the caller.
int launch_ls_prepass(eaqhm_ctx* ctx, LsArgs A, long long track_t0) {
  hipLaunchKernelGGL(eaqhm_ls_classify_kernel, dim3((A.n_frames + 255) / 256), dim3(256), 0, ctx->stream, A);
  HIP_TRY(ctx, hipGetLastError());
  if (A.mode == 1) {
    // only the chunks the resident track window overlaps (a time block of a long file is a small part of the file)
    const int ch0 = (int)(track_t0 >> 10), ch1 = (int)((track_t0 + A.Lt - 1) >> 10);
    hipLaunchKernelGGL(eaqhm_ls_zero_prefix_kernel, dim3(ch1 - ch0 + 1, A.Kmax), dim3(256), 0, ctx->stream, A.fm_cur, A.Lt,
                       track_t0, ch0, A.zchunks, A.zflag, (unsigned short*)A.zloc, (int*)A.ztot);
    HIP_TRY(ctx, hipGetLastError());
  }
  return EAQHM_OK;
}

// A.scratch / A.scratch_stride / A.zloc / A.ztot / A.cls / A.debug are set by the caller (eaqhm_ls_batch), after launch_ls_prepass.
// Returns the largest number of tile rows handled (frames with more are left to the caller's fallback).
int launch_ls_tile(eaqhm_ctx* ctx, LsArgs A, int grid) {
  // adaptation 0: the kernel with two workgroups per CU when its LDS fits, else the mode-0 branch of the tile kernel
  if (A.mode == 0 && ctx->a0_resident && ls_a0tile_fits(A)) return launch_ls_a0tile(ctx, A);
  const int Kcmax = A.Kcmax;
  const int ldx_max = 16 * TL_NTMAX + 16;
  const int TS = 32;
  const size_t lds_bytes = tl_lds_doubles(Kcmax, TS, ldx_max) * sizeof(double);
  if (lds_bytes > TL_LDS_LIMIT) return ctx->fail(EAQHM_EINVAL, "eaqhm_ls_batch: LDS budget exceeded (tile variant)");
  if (!tl_layout_ok(TS, ldx_max)) return ctx->fail(EAQHM_EINVAL, "eaqhm_ls_batch: LDS layout (tile variant)");
  if (a0_lds_doubles(A0_M, 2, TZ_TB, TZ_NCH, 520, 64 * CI_NCH, Kcmax) * sizeof(double) > lds_bytes)
    return ctx->fail(EAQHM_EINVAL, "eaqhm_ls_batch: LDS budget exceeded (adaptation 0, tile variant)");
  HIP_TRY(ctx, hipFuncSetAttribute((const void*)eaqhm_ls_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipLaunchKernelGGL(eaqhm_ls_tile_kernel, dim3(grid), dim3(TL_THREADS), lds_bytes, ctx->stream, A, TS, ldx_max);
  HIP_TRY(ctx, hipGetLastError());
  return EAQHM_OK;
}

}  // namespace eaqhm
