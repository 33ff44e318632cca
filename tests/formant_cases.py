"""Inputs of the formant tests (tests/test_formant_cpu.py, tests/test_gpu_formant.py), and their references from
tests/formant_ref.py, computed once per process and shared.

Root cases: per order p a batch of distinct frames (ROOT_FRAMES names them): random reflection coefficients with
|k| < 0.9, every effective degree pe in {0, 1, p - 1, p} by trailing zeros, a silent frame between live ones, and at
p = 2 a near-double real pair.  A larger batch is `tiled(p, Nf)`: the distinct frames in rotation, so that its reference
is the distinct frames' own.  The builder's condition (asserted by the CPU test): the model finishes every frame within
48 of the 64 steps."""
from functools import lru_cache

import numpy as np

import formant_ref as R

ORDERS = (1, 2, 3, 18, 31, 32, 62, 63)
BATCHES = (1, 3, 4, 5, 65)
ROOT_FRAMES = ("random-a", "silent", "random-b", "pe-1", "pe-p-1", "pe-p", "random-c", "wide", "random-d")
NEAR_DOUBLE = (0.5, 0.5005)          # the real pair of the p = 2 case: 38 steps in the model


def _k_of_real_pair(r1, r2):
    """k_1, k_2 of z^2 + a_1 z + a_2 with the roots r1, r2: k_2 = a_2, a_1 = k_1 (1 + k_2)."""
    a1, a2 = -(r1 + r2), r1 * r2
    return np.array([a1 / (1.0 + a2), a2])


@lru_cache(maxsize=None)
def root_case(p):
    """refl float64[n, p]: the distinct frames of order p in ROOT_FRAMES' order (plus "near-double" at p = 2)."""
    rng = np.random.default_rng(1000 + p)
    rows = []
    for name in ROOT_FRAMES:
        k = rng.uniform(-0.9, 0.9, p)
        if name == "silent":
            k[:] = 0.0
        elif name == "pe-1":
            k[1:] = 0.0
        elif name == "pe-p-1":
            k[p - 1:] = 0.0
        elif name == "wide":
            k = rng.uniform(-0.99, 0.99, p)
        rows.append(k)
    if p == 2:
        rows.append(_k_of_real_pair(*NEAR_DOUBLE))
    out = np.array(rows)
    out.setflags(write=False)
    return out


def tiled(p, Nf):
    """(refl float64[Nf, p], index int[Nf]): frame i is distinct frame index[i] = i mod n."""
    base = root_case(p)
    index = np.arange(Nf) % len(base)
    return np.ascontiguousarray(base[index]), index


@lru_cache(maxsize=None)
def root_reference(p):
    """dict(z64, it64, zld, itld) of root_case(p): the model in float64 and in long double."""
    z64, it64 = R.roots(root_case(p), np.float64)
    zld, itld = R.roots(root_case(p), np.longdouble)
    return dict(z64=z64, it64=it64, zld=zld, itld=itld)


def match(z, ref):
    """The permutation that pairs z[i] with ref[perm[i]] at the least total distance."""
    from scipy.optimize import linear_sum_assignment
    cost = np.abs(np.asarray(z)[:, None] - np.asarray(ref)[None, :]).astype(np.float64)
    rows, cols = linear_sum_assignment(cost)
    perm = np.empty(len(z), np.int64)
    perm[rows] = cols
    return perm


# ---- candidate cases: (name, roots complex128[Nf, p], iters int32[Nf], fs, fmin, fmax, bw_max)
def _value(z, fs):
    f, b, _, _ = R.candidate_values(np.array([[z]]), fs)
    return float(f[0, 0]), float(b[0, 0])


def candidate_cases():
    fs = 16000.0
    up = 0.5j                                    # arg = pi / 2 in any atan2, |z| = 1/2
    f_up, b_up = _value(up, fs)
    frame = np.array([up, 0.6 + 0.3j, -0.3 + 0.6j, 0.6 - 0.3j, 0.7 + 0j])       # 0.5j has the largest bandwidth
    rng = np.random.default_rng(7)
    th = np.sort(np.concatenate((rng.uniform(0.05, 1.5, 5), rng.uniform(1.6, 2.0, 8))))   # five below pi / 2
    many = np.concatenate([rng.uniform(0.9, 0.99, 13) * np.exp(1j * th), [0.95j, 0.9j],        # 0.95j and 0.9j: equal f
                           rng.uniform(0.9, 0.99, 13) * np.exp(-1j * th), [0.5, -0.5, 0.0]])  # p = 31
    many = many[rng.permutation(31)]
    reals = np.array([0.9, -0.9, 0.5, 0.0, 0.0, -0.1], dtype=np.complex128)
    it1 = np.array([5], np.int32)
    cases = [
        ("fmin-edge", frame[None, :], it1, fs, f_up, 5500.0, 1e9),
        ("fmax-edge", frame[None, :], it1, fs, 50.0, f_up, 1e9),
        ("fmin-above-edge", frame[None, :], it1, fs, np.nextafter(f_up, np.inf), 5500.0, 1e9),
        ("fmax-below-edge", frame[None, :], it1, fs, 50.0, np.nextafter(f_up, 0.0), 1e9),
        ("bw-edge", frame[None, :], it1, fs, 50.0, 8000.0, b_up),
        ("bw-below-edge", frame[None, :], it1, fs, 50.0, 8000.0, np.nextafter(b_up, 0.0)),
        ("unit-circle-bw-0", np.array([[1j, 0.6 + 0.8j, 0.3 + 0.1j]]), it1, fs, 50.0, 8000.0, 0.0),
        ("nine-and-more", np.stack([many, np.roll(many, 7), many[::-1]]), np.array([9, 64, 0], np.int32), fs, 50.0,
         5500.0, 1000.0),
        ("none-qualifies", np.stack([many, many]), np.array([3, 3], np.int32), fs, 6000.0, 7000.0, 1.0),
        ("real-roots-only", np.stack([reals] * 5), np.full(5, 2, np.int32), fs, 0.0, 8000.0, 1e9),
        ("unfinished-between", np.stack([many] * 5), np.array([4, R.ITMAX + 1, 4, R.ITMAX + 1, 4], np.int32), fs, 50.0,
         5500.0, 1000.0),
    ]
    return cases


# ---- tracker cases: (name, L float64[T, N, 8], lf float64[T, 8], count int32[T], N, w_jump, absent_cost)
GARBAGE = 12345.0          # what the tables hold beyond a frame's count: finite, and never to be looked at


def _tables(rng, T, N, count, grid, levels=6):
    if grid:                                      # multiples of 2^-10: sums are exact and ties abound
        L = rng.integers(0, levels, (T, N, R.KC)) / 1024.0
        lf = np.sort(rng.integers(0, 5, (T, R.KC)), axis=1) / 1024.0 + 9.0
    else:
        f = np.sort(rng.uniform(200.0, 5000.0, (T, R.KC)), axis=1)
        b = rng.uniform(30.0, 900.0, (T, R.KC))
        ref = np.array([550.0, 1650.0, 2750.0, 3850.0])[:N]
        L = np.abs(f[:, None, :] - ref[None, :, None]) / 1000.0 + (b / f)[:, None, :]
        lf = np.log2(f)
    beyond = np.arange(R.KC)[None, :] >= count[:, None]
    L = np.where(beyond[:, None, :], GARBAGE, L)
    lf = np.where(beyond, GARBAGE, lf)
    return np.ascontiguousarray(L), np.ascontiguousarray(lf)


@lru_cache(maxsize=None)
def tracker_cases(N):
    rng = np.random.default_rng(50 + N)
    cases = []
    for T in (1, 2, 3, 9, 65):
        for grid in (False, True):
            count = rng.integers(0, R.KC + 1, T).astype(np.int32)
            L, lf = _tables(rng, T, N, count, grid)
            cases.append(("T%d-%s" % (T, "grid" if grid else "random"), L, lf, count, N, 1.0 if not grid else 0.5, 2.0))
    T = 9
    full = np.full(T, R.KC, np.int32)
    some = rng.integers(1, R.KC + 1, T).astype(np.int32)
    ends = some.copy()
    ends[0] = ends[-1] = 0
    few = rng.integers(0, N, T).astype(np.int32) if N > 1 else np.zeros(T, np.int32)
    for name, count, grid, wj, absent in (("all-empty", np.zeros(T, np.int32), True, 1.0, 2.0),
                                          ("empty-first-and-last", ends, False, 1.0, 2.0),
                                          ("empty-first-and-last-grid", ends, True, 1.0, 2.0),
                                          ("fewer-than-N", few, True, 1.0, 2.0),
                                          ("full", full, False, 1.0, 2.0),
                                          ("full-grid", full, True, 0.25, 3.0 / 1024.0),
                                          ("absent-cost-0", some, True, 1.0, 0.0),
                                          ("absent-cost-0-random", some, False, 1.0, 0.0),
                                          ("jump-weight-0", some, True, 0.0, 2.0)):
        L, lf = _tables(rng, T, N, count, grid)
        cases.append((name, L, lf, count, N, wj, absent))
    L, lf = _tables(rng, T, N, some, True)
    cases.append(("zero-weights", np.where(L == GARBAGE, GARBAGE, 0.0), lf, some, N, 0.0, 0.0))
    return tuple(cases)


@lru_cache(maxsize=None)
def tracker_reference(N):
    """name -> formant_ref.forward's dict, for every case of tracker_cases(N)."""
    return {c[0]: R.forward(*c[1:]) for c in tracker_cases(N)}


# ---- SA19 through the NumPy stand-in of signal_allpole
@lru_cache(maxsize=None)
def sa19_allpole(order=18, hop=80, preemphasis=0.97):
    """(refl float64[794, order], fs): noise_model_ref.analyse of the pre-emphasised SA19 against zeros."""
    import os
    from scipy.io import wavfile
    import noise_model_ref as NM
    from conftest import GOLDEN
    fs, x = wavfile.read(os.path.join(GOLDEN, "SA19.WAV"))
    s = x / 32768.0
    y = s.copy()
    y[1:] = s[1:] - preemphasis * s[:-1]
    _, refl, _ = NM.analyse(y, hop, order)
    return refl, float(fs)
