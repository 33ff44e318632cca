// Index table of tile_frame's gather (eaqhm_ls_tile.hip): where entry (R, C) of the stacked system Y^H Y lies among the
// G_p tiles in the workgroup's scratch area.  Y = [X_E | n X_E | s] with X = [X_E | s], so the entry is G_p[a][b]: a = R
// (amplitude row), R - Kc (slope row) or Kc (the signal row R = 2 Kc), likewise b for C, p = the number of slope indices
// among R and C.  Tile (I, J), I >= J, of plane q holds G_q[16 I + i][16 J + j] at complex position 16 i + j; entries above
// the tile diagonal are conjugates of stored ones.  In bytes, with PN = 4096 npair and tri(I) = I (I + 1) / 2:
//     a >> 4 >= b >> 4:   4096 (tri(a >> 4) + (b >> 4)) + 256 (a & 15) + 16 (b & 15) + p PN  =  lo(R) + hi(C)
//     otherwise (up):     4096 (tri(b >> 4) + (a >> 4)) + 256 (b & 15) + 16 (a & 15) + p PN  =  lo(C) + hi(R)
// — a sum of one term per index, the same function of R and of C.  One table entry per index of the frame, built once per
// frame; a value of the gather is two table reads (the column's once per slot), a compare, a select and two additions.
// Plain C++ (no HIP types), so that a host program can check it against the rule written out per entry.
#pragma once

#if defined(__HIPCC__)
#define GI_HD __host__ __device__
#else
#define GI_HD
#endif

// Padding (an index beyond the signal's 2 Kc): lo = hi = GI_BIG, and the unsigned minimum with GI_ZCELL sends the value to
// the cell behind the 3 * 21 tiles that holds 0.0 + 0.0j (ls_tile_scratch_stride has room for it).  Tile rows +64 as a row
// and -64 as a column: a padded entry never counts as `up`, its zero keeps its sign.
#define GI_BIG 0x20000000
#define GI_ZCELL (3 * 21 * 4096)

// Packed tables (TWU_PACKED: the last basis tile column E = T - 1 holds [x_e | n x_e], at most 8 live columns): the pair
// (E, J), J < E, has weights 0 and 1 in rows i and i + 8 of plane 0 and weight 2 in row i + 8 of plane 1; the corner (E, E),
// plane 0 only, has entry (i + 8 pa, j + 8 pb), pa + pb = p.  With s = 1 for a slope index: an index of tile E adds 2048 s
// to lo and 128 s to hi, and two cases are off by a constant — the index of the larger tile (in the corner: the row) not a
// slope index, the other one a slope index: + 2048 - PN for a pair (E, J), + 1920 in the corner.  `mask` (all ones for a
// non-slope index of tile E) of the former and `val` of the latter: the correction is mask & val.
struct GatherEntry {
  int lo, hi, trow, tcol;   // first 16 bytes: all that the unpacked classes read
  int mask, val, r0, r1;
};

GI_HD inline GatherEntry gather_entry(int X, int Kc, int npair, int T, bool packed) {
  GatherEntry e;
  const int a = X - (X >= Kc ? Kc : 0);          // X, X - Kc, and Kc for the signal index 2 Kc
  const int s = (X >= Kc && X < 2 * Kc) ? 1 : 0;  // a slope index
  const int t = a >> 4, i = a & 15, PN = 4096 * npair;
  e.lo = 4096 * (t * (t + 1) / 2) + 256 * i + s * PN;
  e.hi = 4096 * t + 16 * i + s * PN;
  e.trow = e.tcol = t;
  e.mask = 0;
  e.val = s ? 2048 - PN : 0;
  if (packed && t == T - 1) {
    e.lo += s * (2048 - PN);
    e.hi += s * (128 - PN);
    e.mask = s ? 0 : -1;
    e.val = s ? 1920 : 0;
  }
  if (X > 2 * Kc) {
    e.lo = e.hi = GI_BIG;
    e.trow = 64; e.tcol = -64;
    e.mask = e.val = 0;
  }
  e.r0 = e.r1 = 0;
  return e;
}

// Byte offset of entry (row, col) from the entries of its two indices; *up: stored as the conjugate.
GI_HD inline unsigned gather_offset(const GatherEntry& row, const GatherEntry& col, bool packed, bool* up) {
  const bool u = row.trow - col.tcol < 0;
  unsigned off = (unsigned)(u ? row.hi + col.lo : row.lo + col.hi);
  if (packed) off += (unsigned)(u ? (col.mask & row.val) : (row.mask & col.val));
  *up = u;
  return off < (unsigned)GI_ZCELL ? off : (unsigned)GI_ZCELL;
}
