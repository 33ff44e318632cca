"""NumPy model of the time alignment: the local cost between two cepstra in float64 and in
np.longdouble, the band layout, the recursion with the tie rule as a plain loop over the band, the backtrack, and a
brute-force enumeration of every monotone path for tiny tables.

Band: half-width r rows of B around the scaled diagonal, centre c_i = (2 i (nB-1) + (nA-1)) // (2 (nA-1)) (0 when
nA = 1); cell (i, j) is in the band iff |j - c_i| <= r and 0 <= j < nB and is stored at [i, j - c_i + r], W = 2 r + 1.
Codes: 0 from (i-1, j-1), 1 from (i-1, j), 2 from (i, j-1), 3 the start; on equal values the lower code wins."""
import numpy as np

INF = float("inf")
NOT_IN_BAND = 255          # the model's back-pointer for a storage cell outside the table


def centres(nA, nB):
    """c_i in Python integers (exact at any size), as int64[nA]."""
    if nA == 1:
        return np.zeros(1, dtype=np.int64)
    return np.array([(2 * i * (nB - 1) + (nA - 1)) // (2 * (nA - 1)) for i in range(nA)], dtype=np.int64)


def min_radius(nA, nB):
    """The smallest r that admits a path from (0, 0) to (nA-1, nB-1)."""
    if nA == 1:
        return nB - 1
    return (nB - 1 + nA - 2) // (nA - 1)


def full_radius(nA, nB):
    return max(nA, nB) - 1


def in_band(nA, nB, r):
    """bool[nA, W]: the storage cells that are cells of the table."""
    j = centres(nA, nB)[:, None] - r + np.arange(2 * r + 1)[None, :]
    return (j >= 0) & (j < nB)


def to_band(dense, r, fill=INF):
    dense = np.asarray(dense)
    nA, nB = dense.shape
    c = centres(nA, nB)
    out = np.full((nA, 2 * r + 1), fill, dtype=dense.dtype)
    for i in range(nA):
        lo, hi = max(0, int(c[i]) - r), min(nB - 1, int(c[i]) + r)
        out[i, lo - int(c[i]) + r:hi - int(c[i]) + r + 1] = dense[i, lo:hi + 1]
    return out


def to_dense(band, nB, fill=INF):
    band = np.asarray(band)
    nA, W = band.shape
    r = (W - 1) // 2
    c = centres(nA, nB)
    out = np.full((nA, nB), fill, dtype=band.dtype)
    for i in range(nA):
        lo, hi = max(0, int(c[i]) - r), min(nB - 1, int(c[i]) + r)
        out[i, lo:hi + 1] = band[i, lo - int(c[i]) + r:hi - int(c[i]) + r + 1]
    return out


def is_empty(C):
    return np.isneginf(np.asarray(C)[:, 0])


def cost(CA, CB, c0_weight=0.0, empty_cost=4.0, dtype=np.float64):
    """Dense d[nA, nB] = c0_weight dC_0^2 + 2 sum_{p>=1} dC_p^2, dC = CA[i] - CB[j], in `dtype`; 0 between two empty
    rows, empty_cost between an empty row and another."""
    CA, CB = np.asarray(CA, dtype=np.float64), np.asarray(CB, dtype=np.float64)
    ea, eb = is_empty(CA), is_empty(CB)
    A = np.where(ea[:, None], 0.0, CA).astype(dtype)
    B = np.where(eb[:, None], 0.0, CB).astype(dtype)
    diff = A[:, None, :] - B[None, :, :]
    sq = diff * diff
    d = dtype(c0_weight) * sq[:, :, 0] + dtype(2.0) * sq[:, :, 1:].sum(axis=2)
    one = ea[:, None] ^ eb[None, :]
    both = ea[:, None] & eb[None, :]
    d = np.where(one, dtype(empty_cost), d)
    return np.where(both, dtype(0.0), d)


def cost_reversed(CA, CB, c0_weight=0.0):
    """The float64 cost of non-empty rows summed from the highest coefficient down: another summation order."""
    diff = np.asarray(CA)[:, None, :] - np.asarray(CB)[None, :, :]
    sq = diff * diff
    acc = np.zeros(sq.shape[:2])
    for p in range(sq.shape[2] - 1, 0, -1):
        acc = acc + sq[:, :, p]
    return 2.0 * acc + c0_weight * sq[:, :, 0]


def dp_band(band, nA, nB, r):
    """The recursion over a band of costs (any dtype with +, <): (D band, ptr uint8 band).  Storage cells outside the
    table keep the input's value in D and NOT_IN_BAND in ptr.  A plain loop, one addition per cell."""
    W = 2 * r + 1
    c = [int(v) for v in centres(nA, nB)]
    inf = band.dtype.type(INF)
    d = band.tolist() if band.dtype == np.float64 else [list(row) for row in band]
    D = [row[:] for row in d]
    ptr = [[NOT_IN_BAND] * W for _ in range(nA)]
    for i in range(nA):
        ci = c[i]
        cu = c[i - 1] if i > 0 else 0
        Di = D[i]
        Du = D[i - 1] if i > 0 else None
        for k in range(max(0, r - ci), min(W, nB - ci + r)):
            j = k + ci - r
            if i == 0 and j == 0:
                ptr[0][k] = 3
                continue                               # D(0,0) = d(0,0)
            ku = j - cu + r                            # column of (i-1, j) in row i-1
            diag = Du[ku - 1] if i > 0 and j > 0 and 0 <= ku - 1 < W else inf
            up = Du[ku] if i > 0 and 0 <= ku < W else inf
            left = Di[k - 1] if j > 0 and k > 0 else inf
            best, code = diag, 0
            if up < best:
                best, code = up, 1
            if left < best:
                best, code = left, 2
            Di[k] = d[i][k] + best
            ptr[i][k] = code
    return np.array(D, dtype=band.dtype), np.array(ptr, dtype=np.uint8)


def backtrack(ptr, nA, nB, r):
    """The path from (0, 0) to (nA-1, nB-1) in forward order, int64[L, 2]."""
    c = centres(nA, nB)
    i, j = nA - 1, nB - 1
    out = []
    while True:
        out.append((i, j))
        if i == 0 and j == 0:
            break
        code = int(ptr[i, j - int(c[i]) + r])
        assert code in (0, 1, 2), (i, j, code)
        if code == 0:
            i, j = i - 1, j - 1
        elif code == 1:
            i -= 1
        else:
            j -= 1
        assert len(out) <= nA + nB
    return np.array(out[::-1], dtype=np.int64)


def align_band(band, nA, nB, r):
    """(path, total, D band, ptr band) of a band of costs."""
    D, ptr = dp_band(np.asarray(band), nA, nB, r)
    return backtrack(ptr, nA, nB, r), D[nA - 1, nB - 1 - int(centres(nA, nB)[nA - 1]) + r], D, ptr


def align(dense, r=None):
    """(path, total, D band, ptr band) of a dense cost table; r=None is the full table."""
    dense = np.asarray(dense)
    nA, nB = dense.shape
    r = full_radius(nA, nB) if r is None else r
    return align_band(to_band(dense, r), nA, nB, r)


def all_paths(nA, nB, r):
    """Every monotone path from (0, 0) to (nA-1, nB-1) inside the band, each as its list of cells."""
    c = centres(nA, nB)
    out = []

    def walk(i, j, cells):
        if not (0 <= i < nA and 0 <= j < nB and abs(j - int(c[i])) <= r):
            return
        cells = cells + [(i, j)]
        if (i, j) == (nA - 1, nB - 1):
            out.append(cells)
            return
        walk(i + 1, j + 1, cells)
        walk(i + 1, j, cells)
        walk(i, j + 1, cells)

    walk(0, 0, [])
    return out


def backward_codes(cells):
    """The back-pointer codes of a path, read from its end to its start."""
    codes = []
    for (i0, j0), (i1, j1) in zip(cells[:-1], cells[1:]):
        codes.append({(1, 1): 0, (1, 0): 1, (0, 1): 2}[(i1 - i0, j1 - j0)])
    return codes[::-1]


def brute_force(dense, r):
    """(the cheapest path under the tie rule, its cost) by enumeration: among the cheapest paths the one whose codes,
    read from the end, come first in lexicographic order (at every cell the lowest code among the predecessors that a
    cheapest path runs through).  Exact for costs whose sums are exact."""
    dense = np.asarray(dense)
    paths = all_paths(dense.shape[0], dense.shape[1], r)
    sums = [sum(dense[i, j] for i, j in p) for p in paths]
    best = min(sums)
    pick = min((backward_codes(p), p) for p, s in zip(paths, sums) if s == best)[1]
    return np.array(pick, dtype=np.int64), best


def path_is_valid(path, nA, nB, r):
    path = np.asarray(path)
    c = centres(nA, nB)
    steps = np.diff(path, axis=0)
    ok_steps = all(tuple(s) in ((1, 1), (1, 0), (0, 1)) for s in steps)
    return (tuple(path[0]) == (0, 0) and tuple(path[-1]) == (nA - 1, nB - 1) and ok_steps
            and bool(np.all(np.abs(path[:, 1] - c[path[:, 0]]) <= r)))


def alignment_index(path, nA):
    path = np.asarray(path)
    return np.array([path[path[:, 0] == i, 1].mean() for i in range(nA)])
