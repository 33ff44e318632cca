"""A spectral conversion trained from speech that is NOT parallel: the INCA iteration (not in the reference).

    nn_splits(nA, nB) -> the split count of eaqhm_nn_rows, a function of the two row counts alone
    nn_work_len(nA, nB, D) -> doubles of its `work`
    nearest_rows(A, B, *, device_index=0) -> (index int64[nA], dist2 float64[nA]): for every row of A the nearest row of B
    conversion_train_nonparallel(X, Y, components=8, *, rounds=8, tol=1e-3, symmetric=True, level=False, iters=20,
                                 em_tol=1e-5, floor=1e-6, init=None, device_index=0)
        -> (conv, info): a static conversion_train map and dict(ix, iy, trace, rounds, best)
    check_nonparallel_arguments: validation, no device work

This module is reached as eaqhm_amd.nonparallel; the package does not re-export it.

The definition is DESIGN.md §12.5, the algorithm INCA (Erro, Moreno & Bonafonte 2010): pair every row with its nearest
neighbour among the other speaker's rows, train the map on those pairs (convert.conversion_train), convert the source rows
with it (convert.conversion_apply) and search again from the converted rows, until the mean squared distance to the
nearest neighbour stops falling.  The search, O(nA nB D), runs in libeaqhm_hip.so (eaqhm_nn_rows); the pairing, a sort of
nA + nB integers, is host NumPy.  There is no CPU path.

What it is not.  INCA assumes that the two speakers' rows are already close enough for the nearest neighbour to be mostly
the same sound; it converges more slowly and to a worse map than training on aligned rows of the same sentences, and it
has been tried here on synthetic rows only.  The distance is the plain Euclidean one on the mapped static columns: no
deltas, no weights, one neighbour, no exclusion of a row's own neighbourhood.
"""
import math

import numpy as np

from . import convert
from .args import _integer, _real, _rows
from .cepstrum import _cepstrum_rows
from .convert import GMM_MAX_COLUMNS, check_conversion_arguments
from .records import _agree, _device

NN_SPLIT_MIN = 4096        # rows of B of a split at least
NN_BLOCKS = 1024           # splits are added until about this many blocks exist
NN_ROWS_MAX = 2 ** 31 - 1
NONPARALLEL_MAX_ROUNDS = 50


def nn_splits(nA, nB):
    """The split count of eaqhm_nn_rows (include/eaqhm_nn.h): min(ceil(nB / 4096), max(1, ceil(1024 / ceil(nA / 64)))), a
    function of nA and nB alone."""
    nA, nB = int(nA), int(nB)
    if not (1 <= nA <= NN_ROWS_MAX and 1 <= nB <= NN_ROWS_MAX):
        raise ValueError("nA and nB must be in [1, 2^31)")
    return min(-(-nB // NN_SPLIT_MIN), max(1, -(-NN_BLOCKS // -(-nA // 64))))


def nn_work_len(nA, nB, D):
    """Doubles of eaqhm_nn_rows' `work`: |b_j|^2 per row of B, then a score and an index per (split, row of A)."""
    return int(nB) + 2 * nn_splits(nA, nB) * int(nA)


def nearest_rows(A, B, *, device_index=0):
    """For every row of `A` float64[nA, D] the nearest row of `B` float64[nB, D] in the Euclidean distance (both finite,
    1 <= D <= 128, the same D): (index int64[nA], dist2 float64[nA]).  index[i] minimises the score |b_j|^2 - 2 a_i . b_j,
    the lowest j on equal scores; dist2[i] = |a_i - b_index[i]|^2 is formed from the two rows themselves, never negative
    and exactly 0 for equal rows.  The same bits on every run.  Both sets are uploaded once."""
    A, B = _rows(A, "A", GMM_MAX_COLUMNS), _rows(B, "B", GMM_MAX_COLUMNS)
    if A.shape[1] != B.shape[1]:
        raise ValueError("A and B must have the same number of columns, got %d and %d" % (A.shape[1], B.shape[1]))
    (nA, D), nB = A.shape, B.shape[0]
    words = nn_work_len(nA, nB, D)
    torch, c, dev = _device(device_index)
    _agree("the splits of the nearest-row search", (c.nn_work_len(nA, nB, D), c.nn_splits(nA, nB)),
           (words, nn_splits(nA, nB)))
    A_d, B_d = torch.as_tensor(A, device=dev), torch.as_tensor(B, device=dev)
    work = torch.empty(words, dtype=torch.float64, device=dev)
    index = torch.empty(nA, dtype=torch.int64, device=dev)
    dist2 = torch.empty(nA, dtype=torch.float64, device=dev)
    c.nn_rows(A_d, nA, D, B_d, nB, D, D, work, index, dist2)
    return index.cpu().numpy(), dist2.cpu().numpy()


def check_nonparallel_arguments(X, Y, components=8, rounds=8, tol=1e-3, symmetric=True, level=False, iters=20,
                                em_tol=1e-5, floor=1e-6, init=None):
    """Validates everything conversion_train_nonparallel gets (no device work): returns (X, Y, rounds, tol, symmetric,
    level) with X, Y float64 cepstral rows.  The training arguments go to convert.check_conversion_arguments with the
    fewest pairs a round can have, one per non-empty row of X.  `init` is None or "kmeans": the pairs change from round to
    round, so labels per pair have no meaning."""
    X, Y = _cepstrum_rows(X, "X"), _cepstrum_rows(Y, "Y")
    if X.shape[1] != Y.shape[1]:
        raise ValueError("X and Y must have the same number of columns (the first search compares them directly), got "
                         "%d and %d" % (X.shape[1], Y.shape[1]))
    nx, ny = (int(np.count_nonzero(~np.isneginf(C[:, 0]))) for C in (X, Y))
    if nx < 1 or ny < 1:
        raise ValueError("X and Y need at least one non-empty row each")
    rounds = _integer(rounds, "rounds")
    if not 1 <= rounds <= NONPARALLEL_MAX_ROUNDS:
        raise ValueError("rounds must be in [1, %d], got %d" % (NONPARALLEL_MAX_ROUNDS, rounds))
    if isinstance(tol, (bool, np.bool_)):
        raise ValueError("tol must be a number")
    tol = _real(tol, "tol", 0.0, 1.0)
    if tol >= 1.0:
        raise ValueError("tol must be in [0, 1), got %r" % (tol,))
    if not isinstance(symmetric, (bool, np.bool_)):
        raise ValueError("symmetric must be True or False")
    if init is not None and not isinstance(init, str):
        raise ValueError('init must be None or "kmeans": the pairs change from round to round')
    stand_in = np.zeros((nx, X.shape[1]))
    _, _, level = check_conversion_arguments(stand_in, stand_in, components, level, iters, em_tol, floor, init, None)
    return X, Y, rounds, tol, bool(symmetric), level


def nonparallel_pairs(p, q=None):
    """The pairs of one round as int64[L, 2], sorted by (k, j) and without duplicates: (k, p[k]) for every k and, with
    `q`, (q[j], j) for every j."""
    p = np.asarray(p, dtype=np.int64)
    pairs = np.column_stack((np.arange(len(p), dtype=np.int64), p))
    if q is not None:
        q = np.asarray(q, dtype=np.int64)
        pairs = np.vstack((pairs, np.column_stack((q, np.arange(len(q), dtype=np.int64)))))
    return np.unique(pairs, axis=0)


def conversion_train_nonparallel(X, Y, components=8, *, rounds=8, tol=1e-3, symmetric=True, level=False, iters=20,
                                 em_tol=1e-5, floor=1e-6, init=None, device_index=0):
    """Learns the map from speaker A's cepstral rows `X` float64[nX, P + 1] to speaker B's `Y` float64[nY, P + 1] when
    the two are NOT recordings of the same sentences (INCA, Erro, Moreno & Bonafonte 2010).  The rows
    are in model_cepstrum's layout with the same number of columns; they need not be as many nor in any order; empty
    rows (-inf, 0, .., 0) are never searched and never matched.  The searched columns are the mapped ones: 1.. with
    level=False, all with level=True.  With xs, ys the non-empty rows' searched columns and xc = xs at first, round r
        pairs every row of xc with its nearest row of ys and, with symmetric=True, every row of ys with its nearest row of
            xc (nearest_rows),
        records trace[r], the mean squared distance over those nx + ny (or nx) searches,
        stops when r >= 1 and trace[r] > (1 - tol) trace[r - 1], or when r = rounds,
        trains conv_(r+1) = conversion_train(X[ix], Y[iy], components, level=, iters=, tol=em_tol, floor=, init=) on the
            pairs, duplicates dropped, sorted by (row of X, row of Y),
        and sets xc to the searched columns of conversion_apply(conv_(r+1), the non-empty rows of X).
    Returns (conv, info).  conv is conv_b, b the r >= 1 of smallest trace[r] (the lowest on ties): a plain static
    conversion_train map, which check_conversion, conversion_apply and np.savez take as it is.  info = dict(ix, iy: int64
    indices into X and Y AS GIVEN of the pairs that trained conv_b; trace float64[r_stop + 1]; rounds, the maps trained;
    best, b).  `rounds` is in [1, 50] and `tol` in [0, 1); 8 and 1e-3 are choices, not optima: on the test set of DESIGN.md
    §12.5 the trace still falls slowly at round 8.  A dynamic map comes from the pairs:
    conversion_train(dynamic_rows(X, 2)[info["ix"]], dynamic_rows(Y, 2)[info["iy"]], span=2), X and Y each one utterance (or
    the deltas taken per utterance before stacking).  LinAlgError from the training passes through."""
    X, Y, rounds, tol, symmetric, level = check_nonparallel_arguments(X, Y, components, rounds, tol, symmetric, level,
                                                                      iters, em_tol, floor, init)
    skip = 0 if level else 1
    gx, gy = (np.flatnonzero(~np.isneginf(C[:, 0])) for C in (X, Y))
    Xf = np.ascontiguousarray(X[gx])
    ys = np.ascontiguousarray(Y[gy, skip:])
    xc = np.ascontiguousarray(Xf[:, skip:])
    trace, maps, trained_on = [], [], []
    while True:
        p, dp = nearest_rows(xc, ys, device_index=device_index)
        q = None
        if symmetric:
            q, dq = nearest_rows(ys, xc, device_index=device_index)
            trace.append((math.fsum(dp) + math.fsum(dq)) / (len(gx) + len(gy)))
        else:
            trace.append(math.fsum(dp) / len(gx))
        r = len(trace) - 1
        if (r >= 1 and trace[r] > (1.0 - tol) * trace[r - 1]) or r == rounds:
            break
        pairs = nonparallel_pairs(p, q)
        ix, iy = gx[pairs[:, 0]], gy[pairs[:, 1]]
        conv = convert.conversion_train(X[ix], Y[iy], components, level=level, iters=iters, tol=em_tol, floor=floor,
                                        init=init, device_index=device_index)
        maps.append(conv)
        trained_on.append((ix, iy))
        xc = np.ascontiguousarray(convert.conversion_apply(conv, Xf, device_index=device_index)[:, skip:])
    trace = np.array(trace)
    best = 1 + int(np.argmin(trace[1:]))
    ix, iy = trained_on[best - 1]
    return maps[best - 1], dict(ix=ix, iy=iy, trace=trace, rounds=len(maps), best=best)
