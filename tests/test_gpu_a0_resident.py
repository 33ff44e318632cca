"""eaqhm_ls_a0tile_kernel (adaptation 0 of the tile classes, two workgroups resident per CU) against the mode-0 branch
of eaqhm_ls_tile_kernel, bit for bit, and against the NumPy model.

Cases: tests/ls_batch_ref.py, _case_Z at fs = 16000, Kmax = 51, frame_K the first and last K of every real tile-row count
m = (2K + 2 + 15) >> 4 = 1..7 — K = 8m - 1 fills the last tile (2K + 2 = 16m), K = 8m leaves it nearly empty — and both of
_case_Z's frames per K.  wl_max = 174 (K = 51, the lower pitch): WP = 176, NP = 352,
    a0res_lds_doubles = max(8 * 7 * 104 + 3 * 176 + 2 * 352, 4 * 7 * 272) + 2 * 896 + 224 + 18 + 4 * 103 = 10230 doubles,
81,840 bytes <= 80 KiB - 16, so the new kernel takes the launch; that it did is read from word 15 of eaqhm_debug_read
(frames it solved), not assumed.  EAQHM_OPT_A0_RESIDENT = 0 and a launch that declares wl_max = 511 go through the tile
kernel and leave that word zero.

Bars: those of tests/test_gpu_ls_batch_direct.py."""
import numpy as np
import pytest

import ls_batch_ref as R

pytestmark = pytest.mark.gpu

TOL_AM_REL, TOL_FM_HZ, TOL_PH_RAD = 1e-8, 1e-3, 1e-5      # tests/test_gpu_ls_batch_direct.py
BAR_AMP, BAR_SLOPE = 1e-9, 1e-8
KS = (1, 7, 8, 15, 16, 23, 24, 31, 32, 39, 40, 47, 48, 51)
OPT_DEBUG_KEEP, OPT_A0_RESIDENT = 2, 4                    # include/eaqhm_hip.h


def wrap(d):
    return (d + np.pi) % (2 * np.pi) - np.pi


@pytest.fixture(scope="module")
def reference():
    """(case, model result): computed once, never changed."""
    case = R._case_Z("ZR", 16000, 51, KS, 12)
    assert case["n_frames"] == 2 * len(KS) and case["wl_max"] <= 174
    assert sorted({t["nt"] for t in case["tags"]}) == list(range(1, 14)) and max(case["frame_K"]) == 51
    with R.one_thread():
        ref = R.run(case)
    return case, ref


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from eaqhm_amd.hip import Context
    c = Context(0)
    yield c
    c.set_option(OPT_DEBUG_KEEP, 0)
    c.set_option(OPT_A0_RESIDENT, 1)


def launch(ctx, case, resident):
    """One launch of the case with EAQHM_OPT_A0_RESIDENT = resident; adds solved = frames eaqhm_ls_a0tile_kernel solved.
    (The debug words live at the end of the context's scratch: a first launch makes it large enough, so that the
    counted one does not move them.)"""
    ctx.set_option(OPT_A0_RESIDENT, resident)
    ctx.set_option(OPT_DEBUG_KEEP, 0)
    R.run(case, ctx)
    ctx.set_option(OPT_DEBUG_KEEP, 1)                       # clears the words
    got = R.run(case, ctx)
    got["solved"] = ctx.debug_read()[15]
    ctx.set_option(OPT_DEBUG_KEEP, 0)
    ctx.set_option(OPT_A0_RESIDENT, 1)
    return got


@pytest.fixture(scope="module")
def launched(ctx, reference):
    cache = {}

    def get(resident):
        if resident not in cache:
            cache[resident] = launch(ctx, reference[0], resident)
        return cache[resident]
    return get


def assert_bars(case, ref, got, frames, src=None):
    """Frames `frames` of launch `got` (frame i of it is frame src[i] of the case and of `ref`) at the bars."""
    src = np.arange(case["n_frames"]) if src is None else np.asarray(src)
    K = case["Kmax"]
    for i in frames:
        f = int(src[i])
        Kc = 2 * int(case["frame_K"][f]) + 1
        for key, bar in (("raw_amp", BAR_AMP), ("raw_slope", BAR_SLOPE)):
            r, g = ref[key][f, :Kc], got[key][i, :Kc]
            e = np.abs(g - r).max() / np.abs(r).max()
            assert np.isfinite(e) and e <= bar, (key, i, f, Kc, e)
            assert np.isnan(got[key][i, Kc:]).all()
    rows = case["frame_inst"][src[np.asarray(frames)]]
    g, r = got["records"][rows], ref["records"][rows]
    assert np.isfinite(g).all() and np.isfinite(r).all()
    mg, mr = g[:, :K] != 0, r[:, :K] != 0
    assert np.mean(mg == mr) >= 0.999
    assert not (g[:, K:3 * K] != 0)[~np.tile(mg, 2)].any()
    both = mg & mr
    top = r[:, :K].max()
    assert np.abs(g[:, :K] - r[:, :K])[both].max() <= TOL_AM_REL * top
    assert np.abs(g[:, K:2 * K] - r[:, K:2 * K])[both].max() <= TOL_FM_HZ
    strong = both & (r[:, :K] > 1e-6 * top)
    assert np.abs(wrap(g[:, 2 * K:3 * K] - r[:, 2 * K:3 * K]))[strong].max() <= TOL_PH_RAD
    assert np.abs(g[:, 3 * K] - r[:, 3 * K]).max() <= TOL_AM_REL * top


def assert_same_bits(a, b):
    assert np.array_equal(a["records"], b["records"], equal_nan=True)
    for key in ("raw_amp", "raw_slope"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_the_new_kernel_takes_the_launch_and_the_option_switches_it_off(reference, launched):
    case = reference[0]
    assert launched(1)["solved"] == case["n_frames"]
    assert launched(0)["solved"] == 0
    assert launched(1)["faults"] == (0, 0, 0) and launched(0)["faults"] == (0, 0, 0)          # check D


def test_bitwise_equal_to_the_tile_kernel(reference, launched):                               # check A
    case = reference[0]
    assert_same_bits(launched(1), launched(0))
    rows = case["frame_inst"]
    assert np.isfinite(launched(1)["records"][rows]).all()
    others = np.setdiff1d(np.arange(case["n_rows"]), rows)
    assert len(others) == 3 and np.isnan(launched(1)["records"][others]).all()


@pytest.mark.parametrize("resident", (1, 0))
def test_every_frame_against_the_model(reference, launched, resident):                        # check B
    case, ref = reference
    assert_bars(case, ref, launched(resident), range(case["n_frames"]))


def test_consecutive_frames_of_other_sizes_in_one_workgroup(ctx, reference):                  # check C
    """2 n_cu + 64 frames on 2 n_cu workgroups: some take a second and a third frame, of another size class, over the
    panels of the one before (the window, the signal and the table work space lie inside the panel region)."""
    case, ref = reference
    nf = 2 * ctx.n_cu + 64
    src = np.arange(nf) % case["n_frames"]
    big = R.reorder(case, src)                              # (frames of one source write the same row with the same values)
    new, old = launch(ctx, big, 1), launch(ctx, big, 0)
    assert new["solved"] == nf and old["solved"] == 0
    assert new["faults"] == (0, 0, 0) and old["faults"] == (0, 0, 0)
    assert_same_bits(new, old)
    assert_bars(case, ref, new, np.linspace(0, nf - 1, 64).astype(int), src)


def test_a_launch_that_does_not_fit_falls_back(ctx, reference):                               # check E
    case, ref = reference
    got = launch(ctx, dict(case, wl_max=511), 1)
    assert got["solved"] == 0 and got["faults"] == (0, 0, 0)
    assert_bars(case, ref, got, range(case["n_frames"]))
