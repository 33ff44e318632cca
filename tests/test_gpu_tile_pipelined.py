"""Last-chunk shapes, the time split of the 8-row class and the gather of eaqhm_ls_tile_kernel's three-weight contraction.

The k-step loops of the contraction (csrc/eaqhm_ls_tile.hip) run only the k-steps of a chunk that hold samples, and in
frames of 8 tile rows with four basis tile columns (T = 4) two of the ten basis pairs are split along time: waves 0/1 and
2/3 take k-steps 0..3 and 4..7 of every chunk of pairs 8 and 9, and the partial tiles are added in a fixed order before
the gather.  Both can only go wrong where a chunk holds fewer than eight k-steps: the last chunk of a window.  (The file
is named after the software-pipelined k-step loops it was written for; they were measured and not kept,
profiles/tw_pipeline/README.md — a read-ahead would go wrong in the same place.)  Raw adaptation-1 solutions of the tile
kernel (variant 3), frame by frame, against eaqhm_ls_mfma_kernel (variant 2) at the tolerances of
test_gpu_tile_threeweight_large.py, whose helpers this file uses, on windows that end on EVERY last-chunk shape:
(wl + 1) mod 16 = r sample pairs in the last chunk (0: a full one), ceil(r / 2) k-steps, 1..8 of them.

Inputs, chosen on the CPU from the frame plan (K and wl of every frame) and asserted below before the GPU is used:
  whole-pair classes (8, 9, 10 tile rows): glide 190 -> 285 Hz, 5 pitch periods per window: wl = 144..205, each of the
      three classes ends on all 16 shapes (with 4 periods the 8-row class misses 5..8) — residues 7, 8 and 9 of the 8-row
      class, on either side of the half boundary at four k-steps, among them;
  unit-table classes (11, 12 tile rows): glide 163 -> 197.5 Hz, 4 pitch periods: wl = 164..196, all 16 shapes in each;
  control (<= 8 tile rows with fewer than four basis tile columns, n <= 23: no split): glide 300 -> 420 Hz, 4 pitch periods.
Every input is analysed once per variant; the tests share the results.  The same launch twice gives the same bits: the
partial tiles of a split pair and the diagonal units' RI - RI^T are combined in a fixed order."""
import numpy as np
import pytest

from test_gpu_tile_threeweight_large import TOL_AMP, TOL_SLOPE, _raw_adaptation1, glide_signal, plan_for

pytestmark = pytest.mark.gpu

INPUTS = {
    "whole_pair": dict(f_lo=190.0, f_hi=285.0, pitch_periods=5),
    "unit_table": dict(f_lo=163.0, f_hi=197.5, pitch_periods=4),
    "control": dict(f_lo=300.0, f_hi=420.0, pitch_periods=4),
}
ALL_SHAPES = set(range(16))
_cache = {}


def tile_rows(ncol):
    return (2 * (2 * np.asarray(ncol) + 1) + 1 + 15) // 16


def last_chunk_pairs(wl):
    return (np.asarray(wl) + 1) % 16


def ksteps_of(residues):
    """k-steps of the last chunk for each number of sample pairs in it (0: a full chunk of 16 pairs)."""
    return {((r or 16) + 1) // 2 for r in residues}


def _input(name):
    if ("in", name) not in _cache:
        a = INPUTS[name]
        s, track = glide_signal(22400, f_lo=a["f_lo"], f_hi=a["f_hi"])
        _cache["in", name] = (s, plan_for(s, track, a["pitch_periods"]))
    return _cache["in", name]


def _raw(name, variant, again=False):
    key = ("raw", name, variant, again)
    if key not in _cache:
        import torch
        assert torch.cuda.is_available(), "these tests need the MI355X"
        s, plan = _input(name)
        _cache[key] = _raw_adaptation1(s, plan, variant)
    return _cache[key]


def _compare(name, lo, hi, frames=None):
    """Frames of lo..hi tile rows (or the given mask) of input `name`: tile kernel against the large-frame kernel."""
    _, plan = _input(name)
    tile, big = _raw(name, 3), _raw(name, 2)
    ncol = tile["ncol"]
    assert len(ncol) == plan.n_frames and np.array_equal(ncol, big["ncol"])
    Kc, nt = 2 * ncol + 1, tile_rows(ncol)
    sel = (nt >= lo) & (nt <= hi) if frames is None else frames(ncol, nt)
    worst = {}
    for f in np.flatnonzero(sel):
        k = Kc[f]
        a, b = tile["amp"][f][:k], big["amp"][f][:k]
        sa, sb = tile["slope"][f][:k], big["slope"][f][:k]
        ea = np.abs(a - b).max() / np.abs(b).max()
        es = np.abs(sa - sb).max() / np.abs(sb).max()
        w = worst.setdefault(int(nt[f]), [0.0, 0.0])
        w[0], w[1] = max(w[0], ea), max(w[1], es)
        assert ea < TOL_AMP and es < TOL_SLOPE, (int(nt[f]), int(f), int(ncol[f]), int(plan.frame_wl[f]), ea, es)
    print("frames per class:", {c: int((sel & (nt == c)).sum()) for c in sorted(set(nt[sel].tolist()))})
    print("worst relative error per class (amplitude, slope):", worst)
    return plan, ncol, nt


def _planned_shapes(name, c):
    """Last-chunk shapes of class c as the plan alone predicts them (no GPU): K harmonics give n = K columns."""
    _, plan = _input(name)
    return set(last_chunk_pairs(plan.frame_wl[tile_rows(plan.frame_K) == c]).tolist())


def test_ksteps_helper():
    assert ksteps_of({1, 2}) == {1} and ksteps_of({7, 8, 9}) == {4, 5} and ksteps_of({15, 0}) == {8}
    assert ksteps_of(ALL_SHAPES) == set(range(1, 9))


def test_whole_pair_classes_every_last_chunk_shape():
    for c in (8, 9, 10):   # on the CPU first: the input is what the docstring says it is
        assert _planned_shapes("whole_pair", c) == ALL_SHAPES, (c, sorted(_planned_shapes("whole_pair", c)))
    plan, ncol, nt = _compare("whole_pair", 7, 10)
    for c in (8, 9, 10):
        got = set(last_chunk_pairs(plan.frame_wl[nt == c]).tolist())
        assert ksteps_of(got) == set(range(1, 9)), (c, sorted(got))
    assert {7, 8, 9} <= set(last_chunk_pairs(plan.frame_wl[nt == 8]).tolist())
    # the 8-row frames of this input have four basis tile columns (ten pairs, two of them in a second slot)
    assert (ncol[nt == 8] >= 24).all()


def test_unit_table_classes_every_last_chunk_shape():
    for c in (11, 12):
        assert _planned_shapes("unit_table", c) == ALL_SHAPES, (c, sorted(_planned_shapes("unit_table", c)))
    plan, ncol, nt = _compare("unit_table", 10, 13)
    for c in (11, 12):
        got = set(last_chunk_pairs(plan.frame_wl[nt == c]).tolist())
        assert ksteps_of(got) == set(range(1, 9)), (c, sorted(got))


def test_control_fewer_than_four_tile_columns():
    _, plan0 = _input("control")
    assert (np.asarray(plan0.frame_K) <= 23).sum() >= 256
    plan, ncol, nt = _compare("control", 0, 0, frames=lambda ncol, nt: (ncol <= 23) & (nt <= 8) & (ncol >= 1))
    few = (ncol <= 23) & (ncol >= 1)
    assert few.sum() >= 256 and (nt[few] <= 8).all() and (((2 * ncol[few] + 1 + 16) >> 4) < 4).all()


@pytest.mark.parametrize("name", ["whole_pair", "unit_table"])
def test_same_launch_twice_same_bits(name):
    one, two = _raw(name, 3), _raw(name, 3, again=True)
    assert np.array_equal(one["ncol"], two["ncol"])
    assert np.array_equal(one["amp"].view(np.float64), two["amp"].view(np.float64))
    assert np.array_equal(one["slope"].view(np.float64), two["slope"].view(np.float64))
