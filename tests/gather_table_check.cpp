// Host check of csrc/eaqhm_ls_gather.h (compiled and run by test_gather_table_cpu.py): for every Kc = 2 n + 1 whose frames
// contract the three-weight Gramian (T <= 6) and every entry (R, C) of every lower tile of the stacked system, the byte
// offset and the conjugation flag that the index table gives against the rule written out per entry, for the plain tile
// layout and (11 tile rows) for the packed one.
#include <cstdio>
#include <cstddef>
#include "eaqhm_ls_gather.h"
// the rule per entry, as tile_frame's gather computed it value by value before the table
static void parent(int R, int C, int Kc, int npair, int T, bool PK, bool* pad_, size_t* byte, bool* lo_) {
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
  const size_t tile = pad ? 0 : (size_t)(q * npair + I * (I + 1) / 2 + J) * 512;
  const int o = pad ? 0 : 2 * (16 * ii + jj);
  *pad_ = pad; *byte = 8 * (tile + o); *lo_ = lo;
}
int main() {
  long n = 0, bad = 0;
  for (int pk = 0; pk < 2; ++pk)
    for (int Kc = 1; Kc <= 95; Kc += 2) {
      const int Ms = 2 * Kc + 1, nt = (Ms + 15) >> 4, T = (Kc + 16) >> 4, npair = T * (T + 1) / 2;
      if (pk && (nt != 11)) continue;
      GatherEntry tab[208];
      for (int X = 0; X < 16 * nt; ++X) tab[X] = gather_entry(X, Kc, npair, T, pk);
      for (int R = 0; R < 16 * nt; ++R)
        for (int C = 0; C < 16 * nt; ++C) {
          if ((C >> 4) > (R >> 4)) continue;
          bool pad, lo, up; size_t byte;
          parent(R, C, Kc, npair, T, pk, &pad, &byte, &lo);
          const unsigned off = gather_offset(tab[R], tab[C], pk, &up);
          ++n;
          const bool ok = pad ? (off == GI_ZCELL && !up) : (off == byte && up == !lo && off + 16 <= (unsigned)GI_ZCELL && off < 3u * npair * 4096);
          if (!ok && bad++ < 10) printf("pk %d Kc %d R %d C %d: pad %d parent %zu lo %d, new %u up %d\n", pk, Kc, R, C, pad, byte, lo, off, up);
        }
      // the always-padded index of an empty slot
      if (tab[16 * nt - 1].lo != GI_BIG) { printf("Kc %d: index 16 nt - 1 not padding\n", Kc); ++bad; }
    }
  printf("%ld entries, %ld wrong\n", n, bad);
  return bad != 0;
}
