"""The gather of eaqhm_ls_tile_kernel's three-weight classes at every column count.

After the contraction every wave gathers its tiles of the stacked system Y^H Y out of the G_p tiles in the workgroup's
scratch area, through an index table with one entry per row / column index of the frame (csrc/eaqhm_ls_gather.h).  What
can go wrong there depends on where the boundaries between amplitude rows, slope rows and the signal row fall inside a
tile — on Kc mod 16 with Kc = 2 n + 1 —, on the class (slots per wave, whole pairs or unit tables) and on the packed
table of 11 tile rows.  So: raw adaptation-1 solutions of the tile kernel (variant 3), frame by frame, against
eaqhm_ls_mfma_kernel (variant 2) at the tolerances of test_gpu_tile_threeweight_large.py, whose helpers this file uses, at
EVERY column count n of every three-weight class:

  A  glide 160 -> 340 Hz, 4 pitch periods per window: n = 23 .. 47, at least 23 frames of each; tile rows 6 .. 12 are
     n = {23}, {24-27}, {28-31}, {32-35}, {36-39}, {40-43}, {44-47}: all four positions of the signal column in every
     class of 7 .. 12 rows, the split class (8 rows with four basis tile columns) and both unit tables;
  B  glide 300 -> 1000 Hz, 3 pitch periods: n = 7 .. 24, at least 16 frames of each, tile rows 2 .. 7: the small frames
     (up to n = 23 fewer than four basis tile columns, no split).

Both statements are asserted from the frame plan on the CPU before the GPU is used.  Each input is analysed once per
variant; the tests share the results.  The same launch twice gives the same bits."""
import numpy as np
import pytest

from test_gpu_tile_threeweight_large import TOL_AMP, TOL_SLOPE, _raw_adaptation1, glide_signal, plan_for

pytestmark = pytest.mark.gpu

INPUTS = {
    "A": dict(f_lo=160.0, f_hi=340.0, pitch_periods=4, n=range(23, 48), frames_per_n=23,
              rows={6: {23}, 7: set(range(24, 28)), 8: set(range(28, 32)), 9: set(range(32, 36)), 10: set(range(36, 40)),
                    11: set(range(40, 44)), 12: set(range(44, 48))}),
    "B": dict(f_lo=300.0, f_hi=1000.0, pitch_periods=3, n=range(7, 25), frames_per_n=16, rows=None),
}
_cache = {}


def tile_rows(ncol):
    return (2 * (2 * np.asarray(ncol) + 1) + 1 + 15) // 16


def _input(name):
    if ("in", name) not in _cache:
        a = INPUTS[name]
        s, track = glide_signal(22400, f_lo=a["f_lo"], f_hi=a["f_hi"])
        _cache["in", name] = (s, plan_for(s, track, a["pitch_periods"]))
    return _cache["in", name]


def _assert_coverage(name, ncol):
    """Every column count of the input, often enough, in the tile-row classes the docstring names."""
    a = INPUTS[name]
    ncol = np.asarray(ncol)
    count = {n: int((ncol == n).sum()) for n in a["n"]}
    assert min(count.values()) >= a["frames_per_n"], count
    nt = tile_rows(ncol)
    if a["rows"] is None:
        sel = (ncol >= a["n"][0]) & (ncol <= a["n"][-1])
        assert set(nt[sel].tolist()) == set(range(2, 8)), sorted(set(nt[sel].tolist()))
        assert (((2 * ncol[sel & (ncol <= 23)] + 1 + 16) >> 4) < 4).all()   # n <= 23: fewer than four basis tile columns, no split
    else:
        for c, ns in a["rows"].items():
            assert set(ncol[nt == c].tolist()) == ns, (c, sorted(set(ncol[nt == c].tolist())))
        for c in range(7, 13):                                         # the signal column at 2, 6, 10 and 14 of the last tile row
            assert {int(2 * (2 * n + 1) - 16 * (c - 1)) for n in a["rows"][c]} == {2, 6, 10, 14}, c
        assert (((2 * ncol[nt == 8] + 1 + 16) >> 4) == 4).all()      # the 8-row frames are the split class


def _raw(name, variant, again=False):
    key = ("raw", name, variant, again)
    if key not in _cache:
        s, plan = _input(name)
        _assert_coverage(name, plan.frame_K)      # on the CPU first: K harmonics give n = K columns
        import torch
        assert torch.cuda.is_available(), "these tests need the MI355X"
        _cache[key] = _raw_adaptation1(s, plan, variant)
    return _cache[key]


@pytest.mark.parametrize("name", ["A", "B"])
def test_plan_covers_every_column_count(name):
    _, plan = _input(name)
    _assert_coverage(name, plan.frame_K)


@pytest.mark.parametrize("name", ["A", "B"])
def test_every_frame_of_every_column_count(name):
    _, plan = _input(name)
    tile, big = _raw(name, 3), _raw(name, 2)
    ncol = tile["ncol"]
    assert len(ncol) == plan.n_frames and np.array_equal(ncol, big["ncol"])
    _assert_coverage(name, ncol)                  # what the kernels saw is what the plan said
    Kc, nt = 2 * ncol + 1, tile_rows(ncol)
    worst, failed = {}, []
    for f in np.flatnonzero((ncol >= INPUTS[name]["n"][0]) & (ncol <= INPUTS[name]["n"][-1])):
        k = Kc[f]
        a, b = tile["amp"][f][:k], big["amp"][f][:k]
        sa, sb = tile["slope"][f][:k], big["slope"][f][:k]
        ea = np.abs(a - b).max() / np.abs(b).max()
        es = np.abs(sa - sb).max() / np.abs(sb).max()
        w = worst.setdefault(int(ncol[f]), [int(nt[f]), 0, 0.0, 0.0])
        w[1], w[2], w[3] = w[1] + 1, max(w[2], ea), max(w[3], es)
        if not (ea < TOL_AMP and es < TOL_SLOPE):
            failed.append((int(ncol[f]), int(nt[f]), int(f), int(plan.frame_wl[f]), ea, es))
    print("input %s: n: [tile rows, frames, worst relative error of the amplitudes, of the slopes]" % name)
    for n in sorted(worst):
        print("  %2d: %s" % (n, worst[n]))
    assert not failed, failed[:8]


@pytest.mark.parametrize("name", ["A", "B"])
def test_same_launch_twice_same_bits(name):
    one, two = _raw(name, 3), _raw(name, 3, again=True)
    assert np.array_equal(one["ncol"], two["ncol"])
    assert np.array_equal(one["amp"].view(np.float64), two["amp"].view(np.float64))
    assert np.array_equal(one["slope"].view(np.float64), two["slope"].view(np.float64))
