"""The classes of 8, 9 and 10 tile rows of eaqhm_ls_tile_kernel contract the three-weight Gramian as whole basis pairs
(unit tables for 8 and 9 tile rows — 8 balanced over the SIMDs, 9 with the last basis tile column packed — were built,
passed this test and measured slower: profiles/tw_small/README.md).  Raw adaptation-1 solutions of the tile kernel
(variant 3), frame by frame, against eaqhm_ls_mfma_kernel (variant 2) at the tolerances of test_gpu_tile_classes.py, for
the frames of 7..10 tile rows — modelled on test_gpu_tile_threeweight_large.py, whose helpers it uses.

Input: the glide 190 -> 285 Hz with 4 pitch periods per window (with 3 the windows sit at the minimum length and do not
cover the last-chunk shapes): K = 27..40, every column count n = 28..39 of the three classes — both ends of each, Kc + 1 = 66
and 72 with two and eight live columns in the last basis tile column of the 9-row class — and windows of each class that end
on last-chunk shapes 0, 1, 2 and 15.  The second case switches the top slot on and off (alternating +-1.2 Hz on the 5 ms
grid): bridged rows share the scratch area that the G_p tiles are written to."""
import numpy as np
import pytest

from test_gpu_tile_threeweight_large import LAST_CHUNK, TOL_AMP, TOL_SLOPE, _raw_adaptation1, gappy_frames, glide_signal, plan_for

pytestmark = pytest.mark.gpu

CLASSES = (8, 9, 10)


def _compare(wobble):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    s, track = glide_signal(22400, f_lo=190.0, f_hi=285.0, wobble=wobble)
    plan = plan_for(s, track, 4)
    tile, big = _raw_adaptation1(s, plan, 3), _raw_adaptation1(s, plan, 2)
    ncol = tile["ncol"]
    assert len(ncol) == plan.n_frames and np.array_equal(ncol, big["ncol"])
    Kc = 2 * ncol + 1
    nt = (2 * Kc + 1 + 15) // 16
    worst = {}
    for f in np.flatnonzero((nt >= 7) & (nt <= 10)):
        k = Kc[f]
        a, b = tile["amp"][f][:k], big["amp"][f][:k]
        sa, sb = tile["slope"][f][:k], big["slope"][f][:k]
        ea = np.abs(a - b).max() / np.abs(b).max()
        es = np.abs(sa - sb).max() / np.abs(sb).max()
        w = worst.setdefault(int(nt[f]), [0.0, 0.0])
        w[0], w[1] = max(w[0], ea), max(w[1], es)
        assert ea < TOL_AMP and es < TOL_SLOPE, (int(nt[f]), int(f), int(ncol[f]), int(plan.frame_wl[f]), ea, es)
    print("frames per class:", {c: int((nt == c).sum()) for c in sorted(set(nt.tolist()))})
    print("worst relative error per class (amplitude, slope):", worst)
    return plan, ncol, nt, tile


def test_every_column_count_and_last_chunk_shape():
    plan, ncol, nt, _ = _compare(0.0)
    assert set(range(28, 40)) <= set(ncol.tolist()), sorted(set(ncol.tolist()))
    for c in CLASSES:
        assert LAST_CHUNK <= set(((plan.frame_wl[nt == c] + 1) % 16).tolist()), c


def test_bridged_slots_in_the_classes():
    plan, ncol, nt, tile = _compare(1.2)
    gap = gappy_frames(tile["fm"], tile["t0"], plan)
    counts = {c: int((gap & (nt == c)).sum()) for c in CLASSES}
    assert min(counts.values()) >= 8, counts
