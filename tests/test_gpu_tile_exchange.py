"""What a frame of eaqhm_ls_tile_kernel leaves in LDS for the next frame of the same workgroup.

The three-weight classes hand their G_p tiles from the waves that contract them to the waves that own the system tiles
through region U of the workgroup's LDS (csrc/eaqhm_ls_tilexch.h), in one to three rounds depending on the number of basis
tile columns T, with the gather's index table and zero cell in the window areas.  A workgroup runs frames of one T after
frames of another, so the rounds of one layout follow the rounds of another in the same bytes.  A frame's bits must not
depend on its neighbours: raw adaptation-1 solutions of inputs A and B of test_gpu_tile_gather.py (22,400 samples,
n = 7 .. 47, T = 1 .. 6), frame by frame under numpy.array_equal, of

  - the whole launch, all classes mixed,
  - the same frames launched class by class (tile rows of the stacked system, as tools/class_probe.py restricts a launch),
  - the same frames once more with the frame list reversed,

and the whole launch against eaqhm_ls_mfma_kernel (variant 2) at the tolerances of test_gpu_tile_threeweight_large.py.
That every T from 3 to 6, the split class (T = 4 in the class of <= 8 tile rows) and both unit tables (11 and 12 tile
rows) occur is asserted from the frame plan on the CPU before the GPU is used."""
import numpy as np
import pytest

from test_gpu_tile_gather import INPUTS, _assert_coverage, _input, tile_rows
from test_gpu_tile_threeweight_large import TOL_AMP, TOL_SLOPE

pytestmark = pytest.mark.gpu

_cache = {}


def _assert_rounds_covered():
    """Inputs A and B together: every number of basis tile columns, the split class and both unit tables."""
    ncol = np.concatenate([np.asarray(_input(name)[1].frame_K) for name in INPUTS])
    for name in INPUTS:
        _assert_coverage(name, _input(name)[1].frame_K)
    Kc = 2 * ncol + 1
    T, nt = (Kc + 16) >> 4, tile_rows(ncol)
    assert set(range(1, 7)) <= set(T.tolist()), sorted(set(T.tolist()))
    for t in (3, 4, 5, 6):                                       # rounds: 1, 1, 2, 3
        assert ((T == t) & (nt <= 12)).sum() >= 16, t
    assert ((nt <= 8) & (T == 4)).any()                          # the split class
    assert ((nt == 9) & (T == 5)).any() and ((nt == 10) & (T == 5)).any()
    assert ((nt == 11) & (T == 6)).any() and ((nt == 12) & (T == 6)).any()   # the packed and the plain unit table


def _launches(name):
    if name in _cache:
        return _cache[name]
    _assert_rounds_covered()                                     # on the CPU first
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from eaqhm_amd.engine import DeviceAnalysis
    s, plan = _input(name)
    eng = DeviceAnalysis(s, s, plan, 70, 1)
    eng.ctx.set_option(1, 3)
    it = eng.adaptations()
    next(it)                          # adaptation 0 enqueued: the tracks that adaptation 1 reads
    eng.ls_stage(1)                   # frame_prep of adaptation 1 (ncol, cols) and its launch; the tracks stay as they are
    torch.cuda.synchronize()
    p, K, nf = plan, plan.Kmax, eng.nf
    ncol = eng.ncol[:nf].cpu().numpy()
    cols = eng.cols[:nf * K].view(-1, K)
    tabs_all = (eng.frame_inst, eng.frame_c, eng.frame_wl, eng.frame_f0, eng.frame_K, eng.ncol)

    def launch(sel, variant=3):
        idx = torch.as_tensor(np.ascontiguousarray(sel), device=eng.s.device)
        tabs = [t[:nf][idx].contiguous() for t in tabs_all]
        cc = cols[idx].contiguous().view(-1)
        raw = [torch.zeros(len(sel), 2 * (2 * K + 1), dtype=torch.float64, device=eng.s.device) for _ in range(2)]
        eng.ctx.set_option(1, variant)
        eng.ctx.ls_batch(1, eng.s, p.L, p.fs, eng.am_cur, eng.fm_cur, eng.track_t0, eng.track_len, K, tabs[0], tabs[1],
                         tabs[2], tabs[3], tabs[4], tabs[5], cc, eng.seeded, eng.any_seed, len(sel), p.wl_max, 1,
                         p.f0_stale, eng.f0min, eng.records[0], raw[0], raw[1])
        eng.ctx.set_option(1, 3)
        torch.cuda.synchronize()
        return raw[0].cpu().numpy(), raw[1].cpu().numpy()

    every = np.arange(nf)
    nt = tile_rows(ncol)
    out = dict(ncol=ncol, nt=nt, whole=launch(every), big=launch(every, variant=2), reversed=launch(every[::-1].copy()),
               classes={int(c): (np.flatnonzero(nt == c), launch(np.flatnonzero(nt == c))) for c in sorted(set(nt.tolist()))})
    assert eng.ctx.ls_faults() == (0, 0, 0)
    _cache[name] = out
    return out


def _differing(a, b):
    """Frames (rows) whose bits differ."""
    return np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).any(axis=1))


def test_plan_covers_every_round_layout():
    _assert_rounds_covered()


@pytest.mark.parametrize("name", ["A", "B"])
def test_class_by_class_same_bits(name):
    r = _launches(name)
    seen = 0
    for c, (sel, part) in r["classes"].items():
        for k in range(2):
            bad = _differing(r["whole"][k][sel], part[k])
            assert bad.size == 0, (c, k, sel[bad][:8].tolist(), r["ncol"][sel[bad]][:8].tolist())
        seen += len(sel)
    assert seen == len(r["ncol"])


@pytest.mark.parametrize("name", ["A", "B"])
def test_reversed_frame_list_same_bits(name):
    r = _launches(name)
    for k in range(2):
        bad = _differing(r["whole"][k], r["reversed"][k][::-1])
        assert bad.size == 0, (k, bad[:8].tolist(), r["ncol"][bad][:8].tolist(), r["nt"][bad][:8].tolist())


@pytest.mark.parametrize("name", ["A", "B"])
def test_whole_launch_against_the_large_frame_kernel(name):
    r = _launches(name)
    amp, slope = (x.view(np.complex128) for x in r["whole"])
    bamp, bslope = (x.view(np.complex128) for x in r["big"])
    ncol = r["ncol"]
    failed, worst = [], [0.0, 0.0]
    for f in np.flatnonzero((ncol >= INPUTS[name]["n"][0]) & (ncol <= INPUTS[name]["n"][-1])):
        k = 2 * ncol[f] + 1
        ea = np.abs(amp[f][:k] - bamp[f][:k]).max() / np.abs(bamp[f][:k]).max()
        es = np.abs(slope[f][:k] - bslope[f][:k]).max() / np.abs(bslope[f][:k]).max()
        worst = [max(worst[0], ea), max(worst[1], es)]
        if not (ea < TOL_AMP and es < TOL_SLOPE):
            failed.append((int(ncol[f]), int(r["nt"][f]), int(f), ea, es))
    print("input %s: worst relative error of the amplitudes %.2e, of the slopes %.2e" % (name, worst[0], worst[1]))
    assert not failed, failed[:8]
