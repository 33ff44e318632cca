// The exchange of the three-weight Gramian tiles through LDS (eaqhm_ls_tile.hip, tile_frame): between the barrier that
// closes the last basis chunk and the barrier in front of the factorisation, region U of the kernel's LDS
// (eaqhm_ls_tilelds.h) is dead, and the waves that contracted the G_p tiles hand them to the waves that own the system
// tiles there instead of through the workgroup's global scratch area.  Plain C++ (no HIP types), so that a host program can
// check the layout.
//
//   exchange area   bytes [0, TX_BYTES) of region U: TX_TILES tiles of 16 x 16 complex values (4096 bytes each)
//   dflag           the step counter of the diagonal pipeline, zeroed ahead of the barrier in front of the factorisation
//                   while other waves still gather: at TX_DFLAG_BYTE, behind the exchange area (TX_DFLAG_CELL bytes with
//                   the diagnostics' word next to it)
//   index table     the gather's table (eaqhm_ls_gather.h, 32 bytes per index, 16 TL_NTMAX indices) in the frame's analysis
//                   window `win`, which nothing reads once the last chunk is built: tx_table_byte(Kcmax) from the start of
//                   region U
//   zero cell       16 bytes that padding indices read, at the start of the signal window `sig`: tx_zcell_byte(Kcmax)
//
// Rounds.  The planes G_0, G_1, G_2 of a frame with T basis tile columns are 3 npair tiles, npair = T (T + 1) / 2: all three
// fit for T <= 4, two for T = 5, one for T = 6 — tx_planes_per_round(T) planes per round, stored plane q in round
// q / planes_per_round at tile (q % planes_per_round) npair + pair.  A round is: stores, barrier, the gather of the entries
// whose stored plane is in the round, barrier.  The stored plane of an entry is the one its byte offset among the 3 npair
// tiles falls in (gather_offset / (4096 npair)): with the packed table that is not the number of slope indices.  Padding
// (offset GI_ZCELL) belongs to round 0 and reads the zero cell.
//
// Banks.  Inside a tile entry (i, j) would lie at 256 i + 16 j: the lanes of a transposed read (an entry above the tile
// diagonal is the conjugate of entry (j, i)) walk down a column, 256 bytes apart, all in the same four of the 64 banks of
// ds_read_b128.  So the 16-byte cell index is XORed with the row index, by writer and reader alike, after the packed
// corrections: tx_swizzle.  A lane group of ds_read_b128 is sixteen lanes of two neighbouring rows of the wave's 4 x 16 lane
// grid, eight columns of either ({0-3, 12-15} of one row and {4-11} of the next, or the other way round).  The system
// index maps to the basis index by a shift (0, -Kc, or the signal's), so the group reads cells (c + s) ^ i and (c' + s) ^ i'
// with c, c' from complementary column sets and i' = i + 1 (mod 16): two lanes can meet in one cell's banks where
// (c + s) ^ (c' + s) = i ^ i': at most TX_MAX_CONFLICT distinct addresses per bank whatever the shifts, straight or
// transposed, where the load's 64 entries come from one stored tile (unswizzled, a transposed load has 8).  A load across a
// boundary of the index map (Kc, 2 Kc, a basis tile's edge) takes its lanes from several stored tiles, whose in-tile
// positions can coincide: at most TX_MAX_CONFLICT_MIXED there (lanes that read the zero cell share one address, a broadcast).
#pragma once
#include "eaqhm_ls_gather.h"
#include "eaqhm_ls_tilelds.h"

#define TX_TILE_BYTES 4096
#define TX_TILES 30
#define TX_BYTES (TX_TILES * TX_TILE_BYTES)
// Dc + DGP_DOUBLES + 128 + 256 of tile_frame's carve-up, in bytes (eaqhm_ls_tile.hip asserts that it agrees)
#define TX_DFLAG_BYTE (8 * (4 * TL_NTMAX * TLL_TILE + 2 * TLL_TILE + 512 + 128 + 256))
#define TX_DFLAG_CELL 16
#define TX_TABLE_BYTES (32 * 16 * TL_NTMAX)
#define TX_MAX_CONFLICT 2
#define TX_MAX_CONFLICT_MIXED 4

GI_HD constexpr inline int tx_planes_per_round(int T) { return T <= 4 ? 3 : T == 5 ? 2 : T == 6 ? 1 : 0; }
GI_HD constexpr inline int tx_rounds(int T) { return T <= 4 ? 1 : T == 5 ? 2 : 3; }
GI_HD constexpr inline int tx_npair(int T) { return T * (T + 1) / 2; }

static_assert(3 * tx_npair(4) * TX_TILE_BYTES <= TX_BYTES, "T = 4: one round");
static_assert(tx_planes_per_round(5) * tx_npair(5) * TX_TILE_BYTES <= TX_BYTES, "T = 5: two planes in a round");
static_assert(tx_planes_per_round(6) * tx_npair(6) * TX_TILE_BYTES <= TX_BYTES, "T = 6: one plane in a round");
static_assert(TX_BYTES <= TX_DFLAG_BYTE, "dflag's cell lies behind the exchange area");
static_assert(TX_DFLAG_BYTE + TX_DFLAG_CELL <= 8 * tl_usize_c(), "dflag's cell lies in region U");
static_assert(TX_TABLE_BYTES <= 8 * 64 * CI_NCH, "the index table fits the analysis window's area");

// where the index table and the zero cell lie, in bytes from the start of region U (win and sig of tile_frame's carve-up)
GI_HD inline size_t tx_table_byte(int Kcmax) { return 8 * (tl_usize_c() + TL_HEAD_DOUBLES + 4 * (size_t)Kcmax + 16); }
GI_HD inline size_t tx_zcell_byte(int Kcmax) { return tx_table_byte(Kcmax) + 8 * 64 * CI_NCH; }

// the cell index XOR the row index (bits 4..7 ^= bits 8..11); tile bases are multiples of 4096 and pass through
GI_HD inline unsigned tx_swizzle(unsigned off) { return off ^ (((off >> 8) & 15u) << 4); }

// Writer: byte address in region U of entry (i, j) of the tile of `pair` = tri(I) + J in stored plane q — rows 0..15 and
// columns 0..15 of the stored tile, whatever a packed table put there — in the round that holds the plane.
GI_HD inline unsigned tx_entry_addr(int q, int pair, int i, int j, int T) {
  const int slot = (q % tx_planes_per_round(T)) * tx_npair(T) + pair;
  return tx_swizzle((unsigned)(TX_TILE_BYTES * slot + 256 * i + 16 * j));
}
GI_HD inline int tx_round_of_plane(int q, int T) { return q / tx_planes_per_round(T); }

// Reader: the round in which the entry with byte offset `off` (gather_offset) is read, and its byte address in that round.
GI_HD inline int tx_round_of(unsigned off, int T) {
  return off >= (unsigned)GI_ZCELL ? 0 : (int)(off / (unsigned)(TX_TILE_BYTES * tx_npair(T))) / tx_planes_per_round(T);
}
// The address that the gather loads from in round `rd`, for every entry: entries of other rounds load the zero cell and
// their value is not taken (*take = false).  base = rd * planes_per_round * 4096 npair and span = planes_per_round * 4096
// npair are wave-uniform; the compare is the unsigned `off - base < span`.
GI_HD inline unsigned tx_read_addr(unsigned off, int T, int rd, unsigned zcell, bool* take) {
  const unsigned span = (unsigned)(tx_planes_per_round(T) * TX_TILE_BYTES * tx_npair(T)), rel = off - (unsigned)rd * span;
  const bool in = rel < span && off < (unsigned)GI_ZCELL;
  *take = in || (rd == 0 && off >= (unsigned)GI_ZCELL);
  return in ? tx_swizzle(rel) : zcell;
}
