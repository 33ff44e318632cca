// Dynamic LDS of eaqhm_ls_tile_kernel (eaqhm_ls_tile.hip): the sizes of the carve-up that tile_frame lays out, and what a
// workgroup keeps from one frame to the next.  Plain C++ (no HIP types), so that a host program can check the budget.
//
//   region U            usize_c: the basis chunk + slot info in the Gramian phase (usize_g), tile storage afterwards
//   TlHead              TL_HEAD_DOUBLES, at tl_head_offset = usize_c: a constant away from the start, so that tile_frame
//                       keeps no pointer to it (its first TL_HEAD_GAP doubles are what usize_g may reach past usize_c)
//   xs, sh, win, sig    4 Kcmax + 16 + 2 * 64 CI_NCH
//   dorig               16 TL_NTMAX
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define TLL_HD __host__ __device__
#else
#define TLL_HD
#endif

#define TL_NTMAX 13
#define CI_STRIDE 20    // per-slot info: 16 chunk carries, qmid, 1/(am_mid+eps), rho.re, rho.im
#define CI_NCH 16
#define TL_NSLOT 52     // slots of a frame: n <= 51 for Kc <= 103
// the tiles of eaqhm_ls_chol.h (TL_TILE, DG_TILE, in doubles; eaqhm_ls_tile.hip asserts that they agree)
#define TLL_TILE (16 * 17)
#define TLL_DG_TILE (2 * 16 * 17)
// dynamic LDS the kernel may ask for: it also has a static __shared__ word (the frame cursor), and dynamic + static must
// fit the 160 KiB of a workgroup
#define TL_LDS_LIMIT (159 * 1024)

// The header of the NEXT frame: in stage 0 of the factorisation, where all waves but two wait at barrier A for the first
// diagonal tile, one of the waiting waves draws the next item of the class from its cursor and fetches the frame's id, its
// scalars and its slot list — the chain of dependent loads that the next frame would otherwise start with.  cls is the
// class the header was drawn for (-1: none), f < 0 says that the class is exhausted.  The slot lists take turns in two
// buffers: the current frame reads its own until its record is written.
#define TL_HEAD_GAP 16
struct TlHead {
  double gap[TL_HEAD_GAP];       // (the slot flags of the set-up phase: region U of that phase is a little longer)
  double fmc[TL_NSLOT];          // centre frequencies of the current frame's gap-free slots (prepare_slots -> write_record)
  unsigned long long t_last;     // diagnostics: the last stamp of the previous frame (0: none)
  int cls, f, n, c, wl, inst, buf, seeds;   // seeds: *any_seed of the launch (set once, by the kernel)
  int cols[2][TL_NSLOT];
  int even[2];                   // (an even number of doubles: what follows keeps its 16-byte alignment)
};
static_assert(sizeof(TlHead) % 16 == 0, "TlHead: a multiple of 16 bytes");
#define TL_HEAD_DOUBLES ((sizeof(TlHead) + 7) / 8)

TLL_HD constexpr inline size_t tl_usize_c() {
  return (size_t)4 * TL_NTMAX * TLL_TILE + 2 * TLL_TILE + 2 * TLL_DG_TILE + 2 * 16 * TL_NTMAX + 32;
}
TLL_HD inline size_t tl_usize_g(int TS, int ldx_max) {
  return (size_t)2 * TS * ldx_max + (size_t)CI_STRIDE * TL_NSLOT + TL_NSLOT * CI_NCH + 32;
}
// where TlHead lies (in doubles)
TLL_HD inline size_t tl_head_offset() { return tl_usize_c(); }
// the Gramian phase's region U ends inside the header's gap at the latest
TLL_HD inline bool tl_layout_ok(int TS, int ldx_max) { return tl_usize_g(TS, ldx_max) <= tl_usize_c() + TL_HEAD_GAP; }
TLL_HD inline size_t tl_lds_doubles(int Kcmax, int TS, int ldx_max) {
  const size_t c = tl_usize_c() + TL_HEAD_DOUBLES, g = tl_usize_g(TS, ldx_max);
  return (c > g ? c : g) + 4 * (size_t)Kcmax + 16 + 2 * 64 * CI_NCH + 16 * TL_NTMAX;
}

// the tile variant needs its LDS budget (which grows with Kmax through the solution vector) to fit
inline bool tl_applicable(int Kcmax, int Nmax) {
  return Nmax <= 64 * CI_NCH && tl_layout_ok(32, 16 * TL_NTMAX + 16) && tl_lds_doubles(Kcmax, 32, 16 * TL_NTMAX + 16) * sizeof(double) <= TL_LDS_LIMIT;
}
