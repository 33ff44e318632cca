"""Deals the units of the three-weight Gramian to the eight waves of eaqhm_ls_tile_kernel, one table per size class that
contracts by units (11 and 12 tile rows), and writes csrc/eaqhm_ls_twunits.h:
    python tools/tw_units_gen.py > eaqhm-analysis-and-synthesis-in-python_amd/csrc/eaqhm_ls_twunits.h
(`python tools/tw_units_gen.py T ACC` prints the MFMA counts of the plain deal of T tile columns under another cap.)

A unit is (basis pair (I, J), I >= J, weight p in 0..2): one 16 x 16 complex tile of G_p = X_I^H diag(n^p) X_J.  Forms:
    K3  three real products, three accumulators (off-diagonal pairs)
    K4  four real products, two accumulators     (off-diagonal pairs)
    H   three real products, two accumulators    (diagonal pairs: Re = RR + II, Im = RI - RI^T taken at the gather)
Every wave has the same slot layout, so that the accumulators of a slot are the same registers on every wave:
UA slots of three accumulators (K3) followed by UB slots of two (H or K4, a flag of the unit), 3 UA + 2 UB <= ACC.
ACC = 20 -> UA = 4, UB = 4;  18 -> 2, 6;  16 -> 0, 8.

Packed tables.  Where the last basis tile column E = T - 1 holds at most 8 live columns x_e (11 tile rows: Kc + 1 = 82..88,
T = 6) the chunk stores it as [x_e | n x_e] and the pairs that touch it become
    edge units (E, J, q), J < E: the tile E^H X_J (q = 0: rows 0..7 weight 0, rows 8..15 weight 1) or E^H (n X_J) (q = 1:
                                  weights 1 and 2), form K3 or K4 — two products in place of three;
    the corner (E, E):            E^H E in form H, all three weights of the pair in one product.

Rules of the deal (checked again by static_assert in the header, per table):
  - every entry of every G_p exactly once, the accumulator cap per wave;
  - MFMAs per k-step of the SIMDs (waves w and w + 4) equal to within one unit (4 MFMAs);
  - the units of a pair on one wave where the slots allow it: the first 3 (UA / 3) slots of three accumulators and the
    first 3 (UB / 3) slots of two hold whole pairs (weights 0, 1, 2 in a row or, in slots of two, the two units of an edge
    pair and an empty slot: the kernel reads and scales their operands once per k-step), the remaining slots take single
    units.
"""
import sys

ACC = 20
# table index -> (tile rows of the class, T, packed)
TABLES = [(12, 6, False), (11, 6, True)]


def layout(acc):
    ub = 8
    ua = 0
    while 3 * (ua + 1) + 2 * (ub - 1) <= acc:
        ua, ub = ua + 1, ub - 1
    return ua, ub


def unit_mfmas(u):
    return 4 if u[3] == 'K4' else 3


class Deal:
    """Units are (I, J, p or q, form, edge).  Every list is dealt in the order given, each item to the wave of the lightest
    SIMD that has room (ties: the lighter wave, then the lower one)."""

    def __init__(self, acc):
        self.ua, self.ub = layout(acc)
        self.ga, self.gb = self.ua // 3, self.ub // 3
        self.grpA = [[] for _ in range(8)]     # groups of up to three units in K3 slots
        self.grpB = [[] for _ in range(8)]     # ... in two-accumulator slots
        self.sglA = [[] for _ in range(8)]     # single units
        self.sglB = [[] for _ in range(8)]

    def mfma(self, w):
        return sum(unit_mfmas(u) for lst in (self.grpA[w], self.grpB[w]) for g in lst for u in g) + \
            sum(unit_mfmas(u) for u in self.sglA[w] + self.sglB[w])

    def simd(self, w):
        return self.mfma(w % 4) + self.mfma(w % 4 + 4)

    def lightest(self, free):
        return min((w for w in range(8) if free(w)), key=lambda w: (self.simd(w), self.mfma(w), w))

    def groups_a(self, groups):
        for g in groups:
            self.grpA[self.lightest(lambda w: len(self.grpA[w]) < self.ga)].append(g)

    def groups_b(self, groups):
        for g in groups:
            self.grpB[self.lightest(lambda w: len(self.grpB[w]) < self.gb)].append(g)

    def singles_a(self, units):
        for u in units:
            self.sglA[self.lightest(lambda w: len(self.sglA[w]) < self.ua - 3 * self.ga)].append(u)

    def singles_b(self, units):
        for u in units:
            self.sglB[self.lightest(lambda w: len(self.sglB[w]) < self.ub - 3 * self.gb)].append(u)

    def rows(self):
        out = []
        for w in range(8):
            ra = [u for g in self.grpA[w] for u in g + [None] * (3 - len(g))]
            rb = [u for g in self.grpB[w] for u in g + [None] * (3 - len(g))]
            a = ra + [None] * (3 * self.ga - len(ra)) + self.sglA[w]
            b = rb + [None] * (3 * self.gb - len(rb)) + self.sglB[w]
            out.append(a + [None] * (self.ua - len(a)) + b + [None] * (self.ub - len(b)))
        return out


def pair(pr, form):
    return [(pr[0], pr[1], p, form, 0) for p in range(3)]


def edge_pair(pr, form):
    return [(pr[0], pr[1], q, form, 1) for q in range(2)]


def deal_plain(T, acc):
    """Every pair whole where the group slots allow it."""
    d = Deal(acc)
    diag = [(i, i) for i in range(T)]
    off = [(i, j) for i in range(T) for j in range(i)]
    assert len(diag) <= 8 * d.gb and 3 * (len(diag) + len(off)) <= 8 * (d.ua + d.ub), "does not fit eight slots per wave"
    nA = min(len(off), 8 * d.ga)                         # off-diagonal pairs that get a K3 group
    nB = min(len(off) - nA, 8 * d.gb - len(diag))        # ... a K4 group
    # heaviest items first
    d.groups_b([pair(pr, 'K4') for pr in off[nA:nA + nB]])
    d.groups_b([pair(pr, 'H') for pr in diag])
    d.groups_a([pair(pr, 'K3') for pr in off[:nA]])
    rest = [(pr[0], pr[1], p) for pr in off[nA + nB:] for p in range(3)]   # the remainder: pairs split into single units
    n3 = min(len(rest), 8 * (d.ua - 3 * d.ga))
    d.singles_b([u + ('K4', 0) for u in rest[n3:]])
    d.singles_a([u + ('K3', 0) for u in rest[:n3]])
    return d


def deal_packed(T, acc):
    """The last tile column packed: edge pairs of two units, the corner a single H unit."""
    d = Deal(acc)
    E = T - 1
    diag = [(i, i) for i in range(E)]
    off = [(i, j) for i in range(E) for j in range(i)]
    edge = [(E, j) for j in range(E)]
    nA = min(len(off), 8 * d.ga)
    nB = min(len(off) - nA, 8 * d.gb - len(diag))
    assert nA + nB == len(off), "off-diagonal pairs beyond the group slots"
    eB = min(len(edge), 8 * d.gb - len(diag) - nB)      # edge pairs in the K4 group slots that are left
    d.groups_b([pair(pr, 'K4') for pr in off[nA:]])
    d.groups_a([pair(pr, 'K3') for pr in off[:nA]])
    d.groups_b([pair(pr, 'H') for pr in diag])
    d.groups_b([edge_pair(pr, 'K4') for pr in edge[:eB]])
    rest = [u for pr in edge[eB:] for u in edge_pair(pr, 'K3')]
    assert len(rest) <= 8 * (d.ua - 3 * d.ga), "edge units beyond the single K3 slots"
    d.singles_a(rest)
    d.singles_b([(E, E, 0, 'H', 1)])
    return d


def deal_class(T, packed, acc=ACC):
    return deal_packed(T, acc) if packed else deal_plain(T, acc)


FORM = {'K3': 0, 'K4': 1, 'H': 2}


def encode(u):
    return 0xFFFF if u is None else (u[4] << 12) | (u[0] << 8) | (u[1] << 4) | (u[2] << 2) | FORM[u[3]]


def tables():
    """[(tile rows, T, packed, Deal)] in the order of TABLES."""
    return [(rows, T, packed, deal_class(T, packed)) for rows, T, packed in TABLES]


CHECKS = """// ---- the rules of the deal, checked at compile time for every table
constexpr int twu_mfmas(int tb, int w) {   // MFMAs per k-step of wave w
  int m = 0;
  for (int s = 0; s < TWU_UA + TWU_UB; ++s)
    if (TWU_MAPS[tb][w][s] != 0xFFFF) m += ((TWU_MAPS[tb][w][s] & 3) == 1) ? 4 : 3;
  return m;
}
constexpr int twu_count(int tb, int key) {   // how often the unit `key` (a table word without its form) appears
  int c = 0;
  for (int w = 0; w < 8; ++w)
    for (int s = 0; s < TWU_UA + TWU_UB; ++s)
      if (TWU_MAPS[tb][w][s] != 0xFFFF && (TWU_MAPS[tb][w][s] & ~3) == key) ++c;
  return c;
}
// Every entry of every G_p from exactly one unit: a plain pair has its three weights; a packed edge pair its two units
// (q = 0: weights 0 and 1, q = 1: weights 1 and 2 — the gather takes weight 1 from q = 0); the packed corner holds all three.
constexpr bool twu_every_entry_once(int tb) {
  const int T = TWU_TT[tb], E = T - 1;
  const bool pk = TWU_PACKED[tb];
  int live = 0;
  for (int w = 0; w < 8; ++w)
    for (int s = 0; s < TWU_UA + TWU_UB; ++s)
      if (TWU_MAPS[tb][w][s] != 0xFFFF) ++live;
  if (live != (pk ? 3 * E * (E + 1) / 2 + 2 * E + 1 : 3 * T * (T + 1) / 2)) return false;
  for (int I = 0; I < T; ++I)
    for (int J = 0; J <= I; ++J) {
      const int key = (I << 8) | (J << 4);
      if (pk && I == E) {
        if (twu_count(tb, 0x1000 | key) != 1) return false;
        if (J < E && twu_count(tb, 0x1000 | key | (1 << 2)) != 1) return false;
      } else {
        for (int p = 0; p < 3; ++p)
          if (twu_count(tb, key | (p << 2)) != 1) return false;
      }
    }
  return true;
}
// K3 in the three-accumulator slots only, H / K4 in the others, H on diagonal pairs only; the edge flag on the pairs of
// the last tile column of a packed table and nowhere else
constexpr bool twu_forms_fit_slots(int tb) {
  for (int w = 0; w < 8; ++w)
    for (int s = 0; s < TWU_UA + TWU_UB; ++s) {
      const int c = TWU_MAPS[tb][w][s];
      if (c == 0xFFFF) continue;
      const int form = c & 3, I = (c >> 8) & 15, J = (c >> 4) & 15, p = (c >> 2) & 3;
      const bool edge = (c & 0x1000) != 0;
      if ((c & ~0x1FFF) || form > 2 || p == 3 || I >= TWU_TT[tb] || J > I) return false;
      if ((s < TWU_UA) != (form == 0)) return false;
      if ((form == 2) != (I == J)) return false;
      if (edge != (TWU_PACKED[tb] && I == TWU_TT[tb] - 1)) return false;
      if (edge && p > (I == J ? 0 : 1)) return false;
    }
  return true;
}
constexpr bool twu_simds_balanced(int tb) {   // waves w and w + 4 share a SIMD: their MFMAs per k-step, to within one unit
  int lo = 1 << 30, hi = 0;
  for (int w = 0; w < 4; ++w) {
    const int m = twu_mfmas(tb, w) + twu_mfmas(tb, w + 4);
    lo = m < lo ? m : lo;
    hi = m > hi ? m : hi;
  }
  return hi - lo <= 4;
}
// the first 3 (TWU_UA / 3) and 3 (TWU_UB / 3) slots of either kind: whole pairs, p = 0, 1, 2, or an edge pair, q = 0, 1,
// and an empty slot
constexpr bool twu_pairs_whole(int tb) {
  for (int w = 0; w < 8; ++w)
    for (int k = 0; k < 2; ++k) {
      const int s0 = k ? TWU_UA : 0, ng = (k ? TWU_UB : TWU_UA) / 3;
      for (int g = 0; g < ng; ++g) {
        const int c = TWU_MAPS[tb][w][s0 + 3 * g];
        const bool edge = c != 0xFFFF && (c & 0x1000);
        if (edge && (k == 0 || ((c >> 8) & 15) == ((c >> 4) & 15))) return false;   // edge pairs: slots of two; the corner: a single unit
        for (int p = 0; p < 3; ++p)
          if (TWU_MAPS[tb][w][s0 + 3 * g + p] != ((c == 0xFFFF || (edge && p == 2)) ? 0xFFFF : c + (p << 2))) return false;
      }
    }
  return true;
}
static_assert(3 * TWU_UA + 2 * TWU_UB <= TWU_ACC, "accumulator cap per wave");
%s
}  // namespace eaqhm"""


def header():
    ua, ub = layout(ACC)
    out = []
    out.append("// eaqhm_ls_twunits.h — GENERATED by tools/tw_units_gen.py (do not edit): which wave of eaqhm_ls_tile_kernel contracts")
    out.append("// which unit of the three-weight Gramian, one table per size class (TWU_TB_<tile rows>).  A unit is (basis pair (I, J),")
    out.append("// I >= J, weight p): the tile G_p[I][J] = X_I^H diag(n^p) X_J.  TWU_MAPS[table][wave][slot] = (I << 8) | (J << 4) | (p << 2) | form,")
    out.append("// form 0 = K3 (three real products, three accumulators), 1 = K4 (four products, two accumulators), 2 = H (diagonal pair:")
    out.append("// three products, two accumulators, Im = RI - RI^T at the gather); 0xFFFF = empty slot.  Every wave has TWU_UA slots of")
    out.append("// three accumulators (K3 only) followed by TWU_UB slots of two (H or K4): 3 TWU_UA + 2 TWU_UB <= TWU_ACC accumulators.")
    out.append("// The first 3 (TWU_UA / 3) and 3 (TWU_UB / 3) slots of either kind hold whole pairs (p = 0, 1, 2), the others single units.")
    out.append("// Packed tables (TWU_PACKED): the last basis tile column E = T - 1 is stored as [x_e | n x_e] (at most 8 live columns) and")
    out.append("// its pairs carry bit 12: an edge unit (E, J, q) in the p field, J < E, is E^H X_J (q = 0: rows 0..7 weight 0, rows 8..15")
    out.append("// weight 1) or E^H (n X_J) (q = 1: weights 1 and 2); the corner (E, E), form H, is E^H E with all three weights.  An edge")
    out.append("// pair in group slots (two-accumulator slots only) is its two units and an empty slot.")
    out.append("#pragma once")
    out.append("namespace eaqhm {")
    out.append("#define TWU_ACC %d" % ACC)
    out.append("#define TWU_UA %d" % ua)
    out.append("#define TWU_UB %d" % ub)
    out.append("#define TWU_NTB %d" % len(TABLES))
    for i, (rows, T, packed) in enumerate(TABLES):
        out.append("#define TWU_TB_%d %d" % (rows, i))
    out.append("__device__ constexpr int TWU_TT[TWU_NTB] = {%s};            // basis tile columns" % ", ".join(str(t[1]) for t in TABLES))
    out.append("__device__ constexpr bool TWU_PACKED[TWU_NTB] = {%s};" % ", ".join("true" if t[2] else "false" for t in TABLES))
    out.append("__device__ constexpr unsigned short TWU_MAPS[TWU_NTB][8][TWU_UA + TWU_UB] = {")
    for rows, T, packed, d in tables():
        tot = sum(d.mfma(w) for w in range(8))
        out.append("  // %d tile rows: T = %d%s.  MFMAs per k-step: %d in all; per wave %s; per SIMD (waves w, w + 4) %s" %
                   (rows, T, ", packed" if packed else "", tot, " ".join(str(d.mfma(w)) for w in range(8)),
                    " ".join(str(d.simd(w)) for w in range(4))))
        out.append("  {")
        for w, sl in enumerate(d.rows()):
            out.append("    {%s},   // wave %d: %d MFMAs" % (", ".join("0x%04X" % encode(u) for u in sl), w, d.mfma(w)))
        out.append("  },")
    out.append("};")
    both = lambda fn: " && ".join("%s(TWU_TB_%d)" % (fn, t[0]) for t in TABLES)
    out.append(CHECKS % "\n".join('static_assert(%s, "%s");' % (both(fn), msg) for fn, msg in (
        ("twu_pairs_whole", "whole pairs in the group slots"),
        ("twu_every_entry_once", "every entry of every G_p from exactly one unit"),
        ("twu_forms_fit_slots", "unit forms against the slot layout"),
        ("twu_simds_balanced", "MFMAs per k-step of the four SIMDs equal to within one unit"))))
    return "\n".join(out) + "\n"


def main():
    if len(sys.argv) > 2:
        d = deal_plain(int(sys.argv[1]), int(sys.argv[2]))
        print("T = %s, cap %s: %d MFMAs per k-step; per SIMD %s" % (sys.argv[1], sys.argv[2], sum(d.mfma(w) for w in range(8)),
                                                                     " ".join(str(d.simd(w)) for w in range(4))))
        return
    sys.stdout.write(header())


if __name__ == "__main__":
    main()
