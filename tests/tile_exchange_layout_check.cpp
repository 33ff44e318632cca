// Host check of csrc/eaqhm_ls_tilexch.h (compiled and run by test_tile_exchange_layout_cpu.py): the LDS exchange of the
// three-weight Gramian tiles, for every Kc = 2 n + 1, n = 1 .. 47, with the plain tile layout and (11 tile rows) with the
// packed one.  Writer map and reader map are derived here, independently of the header, from the rule in the header comment
// of csrc/eaqhm_ls_gather.h: where the contraction's waves put G_q[a][b], and which G_q[a][b] entry (R, C) of the stacked
// system is.
#include <cstdio>
#include <cstddef>
#include <map>
#include <set>
#include <tuple>
#include "eaqhm_ls_tilexch.h"

typedef std::tuple<int, int, int, int, int> Id;   // stored plane, I, J, row, column of the stored tile

// the rule per entry: which stored tile entry holds (R, C) of the stacked system, or its conjugate partner (`lo` false)
static void rule(int R, int C, int Kc, int T, bool PK, bool* pad_, Id* id, bool* lo_) {
  const bool pad = R > 2 * Kc || C > 2 * Kc;
  const bool rs = R >= Kc && R < 2 * Kc, cs = C >= Kc && C < 2 * Kc;
  const int a = (R == 2 * Kc) ? Kc : rs ? R - Kc : R, b = (C == 2 * Kc) ? Kc : cs ? C - Kc : C;
  const int p = (int)rs + (int)cs;
  const bool lo = (a >> 4) >= (b >> 4);
  const int I = lo ? (a >> 4) : (b >> 4), J = lo ? (b >> 4) : (a >> 4);
  const int i = lo ? (a & 15) : (b & 15), j = lo ? (b & 15) : (a & 15);
  const bool edge = PK && I == T - 1;
  const int q = (edge && I != J) ? (int)(p == 2) : edge ? 0 : p;
  const int ii = edge ? i + ((I != J) ? 8 * (p - q) : (p >= 1 ? 8 : 0)) : i;
  const int jj = (edge && I == J && p == 2) ? j + 8 : j;
  *pad_ = pad; *id = Id(q, I, J, ii, jj); *lo_ = lo;
}

// the four lane groups of ds_read_b128, one LDS cycle each when conflict-free; bank of byte address a: (a / 4) mod 64
static const int GROUPS[4][16] = {
  {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
  {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
  {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
  {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

// most distinct addresses of one lane group that share a bank (a 16-byte read covers four banks: (a / 16) mod 16 names them)
static int degree(const unsigned* addr) {
  int worst = 0;
  for (int g = 0; g < 4; ++g) {
    std::set<unsigned> per[16];
    for (int k = 0; k < 16; ++k) per[(addr[GROUPS[g][k]] >> 4) & 15].insert(addr[GROUPS[g][k]]);
    for (int b = 0; b < 16; ++b) worst = (int)per[b].size() > worst ? (int)per[b].size() : worst;
  }
  return worst;
}

int main() {
  long n = 0, bad = 0;
  int deg_straight = 0, deg_up = 0, deg_mixed = 0, deg_up_plain = 0;
  for (int pk = 0; pk < 2; ++pk)
    for (int Kc = 3; Kc <= 95; Kc += 2) {
      const int Ms = 2 * Kc + 1, nt = (Ms + 15) >> 4, T = (Kc + 16) >> 4, npair = T * (T + 1) / 2, E = T - 1;
      if (pk && nt != 11) continue;
      const int NR = tx_rounds(T), PPR = tx_planes_per_round(T);
      if (npair != tx_npair(T) || PPR * NR < 3) { printf("Kc %d: rounds\n", Kc); ++bad; continue; }
      // where the table, the zero cell and dflag's cell lie: a launch whose largest frame is this one, and the largest launch
      for (int Kcmax : {Kc, 103}) {
        const size_t tb = tx_table_byte(Kcmax), zc = tx_zcell_byte(Kcmax);
        const bool ok = tb >= 8 * (tl_usize_c() + TL_HEAD_DOUBLES) && tb >= (size_t)TX_BYTES && zc >= tb + TX_TABLE_BYTES &&
                        tb % 16 == 0 && zc % 16 == 0 &&
                        zc + 16 <= 8 * (tl_lds_doubles(Kcmax, 32, 16 * TL_NTMAX + 16) - 16 * TL_NTMAX) &&
                        (size_t)TX_DFLAG_BYTE >= (size_t)TX_BYTES && (size_t)TX_DFLAG_BYTE + TX_DFLAG_CELL <= 8 * tl_usize_c();
        if (!ok) { printf("Kc %d Kcmax %d: table %zu zero cell %zu\n", Kc, Kcmax, tb, zc); ++bad; }
      }
      const unsigned zcell = (unsigned)tx_zcell_byte(103);
      // ---- writer: every stored tile entry of every stored plane, in its round
      std::map<unsigned, Id> written[3];
      for (int I = 0; I < T; ++I)
        for (int J = 0; J <= I; ++J)
          for (int q = 0; q < 3; ++q) {
            if (pk && I == E && q > (I == J ? 0 : 1)) continue;   // packed: two edge units per pair, one corner
            for (int i = 0; i < 16; ++i)
              for (int j = 0; j < 16; ++j) {
                const unsigned ad = tx_entry_addr(q, I * (I + 1) / 2 + J, i, j, T);
                const int rd = tx_round_of_plane(q, T);
                ++n;
                if (rd < 0 || rd >= NR || ad % 16 || ad + 16 > (unsigned)TX_BYTES || written[rd].count(ad)) {
                  if (bad++ < 10) printf("pk %d Kc %d: store q %d (%d, %d) entry (%d, %d) at %u round %d\n", pk, Kc, q, I, J, i, j, ad, rd);
                  continue;
                }
                written[rd][ad] = Id(q, I, J, i, j);
              }
          }
      // ---- reader: every entry of every lower tile of the stacked system
      GatherEntry tab[16 * TL_NTMAX];
      for (int X = 0; X < 16 * nt; ++X) tab[X] = gather_entry(X, Kc, npair, T, pk);
      for (int R = 0; R < 16 * nt; ++R)
        for (int C = 0; C < 16 * nt; ++C) {
          if ((C >> 4) > (R >> 4)) continue;
          bool pad, lo, up; Id id;
          rule(R, C, Kc, T, pk, &pad, &id, &lo);
          const unsigned off = gather_offset(tab[R], tab[C], pk, &up);
          int taken = 0;
          bool ok = true;
          for (int rd = 0; rd < NR; ++rd) {
            bool take;
            const unsigned ad = tx_read_addr(off, T, rd, zcell, &take);
            ok = ok && (ad == zcell || ad + 16 <= (unsigned)TX_BYTES);   // region U's exchange area or the zero cell, never else
            if (!take) { ok = ok && ad == zcell; continue; }
            ++taken;
            if (pad) { ok = ok && ad == zcell && !up; continue; }
            const auto w = written[rd].find(ad);
            ok = ok && rd == tx_round_of(off, T) && rd == std::get<0>(id) / PPR && up == !lo && w != written[rd].end() && w->second == id;
          }
          ++n;
          if (!(ok && taken == 1) && bad++ < 10)
            printf("pk %d Kc %d R %d C %d: off %u pad %d taken %d\n", pk, Kc, R, C, off, pad, taken);
        }
      // ---- banks: the four loads of every lower system tile, lane (lq, lcol) reads (16 P + lq + 4 r, 16 Q + lcol)
      for (int P = 0; P < nt; ++P)
        for (int Q = 0; Q <= P; ++Q)
          for (int r = 0; r < 4; ++r)
            for (int rd = 0; rd < NR; ++rd) {
              unsigned addr[64], plain[64];
              int ups = 0, takes = 0;
              std::set<unsigned> tiles;   // stored tiles that the load touches
              for (int l = 0; l < 64; ++l) {
                const int R = 16 * P + (l >> 4) + 4 * r, C = 16 * Q + (l & 15);
                bool up, take;
                const unsigned off = gather_offset(tab[R], tab[C], pk, &up);
                addr[l] = tx_read_addr(off, T, rd, zcell, &take);
                plain[l] = (take && off < (unsigned)GI_ZCELL) ? off : zcell;
                ups += up; takes += take && off < (unsigned)GI_ZCELL;
                tiles.insert(off >> 12);
              }
              if (!takes) continue;
              const int d = degree(addr);
              if (takes == 64 && tiles.size() == 1 && ups == 0) deg_straight = d > deg_straight ? d : deg_straight;
              else if (takes == 64 && tiles.size() == 1 && ups == 64) { deg_up = d > deg_up ? d : deg_up; const int dp = degree(plain); deg_up_plain = dp > deg_up_plain ? dp : deg_up_plain; }
              else deg_mixed = d > deg_mixed ? d : deg_mixed;
            }
    }
  printf("conflict degree: straight %d, transposed %d (unswizzled %d), tiles across a boundary %d\n", deg_straight, deg_up, deg_up_plain, deg_mixed);
  if (deg_straight > TX_MAX_CONFLICT || deg_up > TX_MAX_CONFLICT || deg_mixed > TX_MAX_CONFLICT_MIXED) { printf("conflict degree above the documented one\n"); ++bad; }
  printf("%ld entries, %ld wrong\n", n, bad);
  return bad != 0;
}
