"""The serial phases of a frame of eaqhm_ls_tile_kernel: the head (the next frame's header, fetched by a waiting wave
during stage 0 of the factorisation; the slot set-up), the back substitution (row shifts and row swaps in place of
ds_bpermute) and the record row (put together in LDS, centre frequencies kept from the slot set-up).

Inputs A (n = 23..47, tile rows 6..12) and B (n = 7..24, tile rows 2..7) of tests/test_gpu_tile_gather.py, 1430 frames each.
Each is analysed up to the start of adaptation 1 once; the tests then launch eaqhm_ls_batch themselves, on all of the
frames or on a few, with record rows of their own (row i for frame i of the launch, one spare row) pre-set to NaN.

  values    every frame against the large-frame kernel (variant 2): raw solutions at 1e-9 / 1e-8 (test_gpu_tile_gather.py),
            record rows at the bars of tests/test_gpu_ls_batch_direct.py; no faults; the same launch twice, the same bits
  hand-out  small batches of input A: every frame done exactly once (the rows that lost the NaN are the frames' rows, and
            they are bit for bit what the full launch wrote for those frames)
  paths     bridged slots (the wobbling track of test_gpu_tile_threeweight_large.py, sets G and E of ls_batch_ref.py: small
            frames, any_seed through the header's flag); a seeded batch of 11 tile rows, the one class whose record takes
            the centre frequencies kept by the slot set-up — slot 0 active AND seeded at the frame centre, where the kept
            track value would be 37 .. 50 Hz off the 140 Hz that the record must show; and mode 0 through this kernel, where
            no header is ever fetched, bit-equal to eaqhm_ls_a0tile_kernel
  host      the LDS budget with the header in it (LDS_CHECK below, compiled against csrc/eaqhm_ls_tilelds.h; no GPU)

The class cursors (LsArgs::cls[8..14]) live in the context's scratch area and the C ABI does not show them, so that they
end at or above the class counts is not read back here; a frame handed out twice or not at all shows in the rows."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ls_batch_ref as R

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc")
TOL_AMP, TOL_SLOPE = 1e-9, 1e-8                           # tests/test_gpu_tile_gather.py
TOL_AM_REL, TOL_FM_HZ, TOL_PH_RAD = 1e-8, 1e-3, 1e-5      # tests/test_gpu_ls_batch_direct.py
_cache = {}
# host program: the LDS budget of eaqhm_ls_tile_kernel from csrc/eaqhm_ls_tilelds.h (plain C++)
LDS_CHECK = r"""
#include <cstdio>
#include "eaqhm_ls_tilelds.h"

int main() {
  int wrong = 0;
  const int TS = 32, ldx_max = 16 * TL_NTMAX + 16;
  // the carve-up at the largest system of the tile classes and the longest window
  const size_t head = tl_head_offset(), all = tl_lds_doubles(103, TS, ldx_max);
  std::printf("Kcmax 103: header at %zu doubles, %zu doubles = %zu bytes of %d\n", head, all, all * sizeof(double), TL_LDS_LIMIT);
  wrong += !(sizeof(TlHead) % 8 == 0 && TL_HEAD_DOUBLES * 8 == sizeof(TlHead));
  wrong += !(all * sizeof(double) <= TL_LDS_LIMIT);
  wrong += !tl_applicable(103, 1024);
  wrong += tl_applicable(103, 1025);                       // a window longer than 64 CI_NCH samples
  // the header lies behind the tile storage; region U of the Gramian phase (a little longer) ends inside the header's gap,
  // ahead of anything the header keeps; the rest of the persistent part follows the header
  const size_t c = tl_usize_c(), g = tl_usize_g(TS, ldx_max);
  wrong += !(head == c && tl_layout_ok(TS, ldx_max) && g <= c + TL_HEAD_GAP && g > c);
  wrong += !(offsetof(TlHead, fmc) == TL_HEAD_GAP * sizeof(double));
  wrong += !(all == c + TL_HEAD_DOUBLES + 4 * 103 + 16 + 2 * 64 * CI_NCH + 16 * TL_NTMAX);
  wrong += tl_layout_ok(TS, ldx_max + 16);                 // a longer chunk row would reach into the header
  // tl_applicable is the budget and nothing else: it flips exactly where the bytes cross the limit
  int flips = 0;
  for (int Kc = 1; Kc <= 4001; Kc += 2) {
    const bool fits = tl_lds_doubles(Kc, TS, ldx_max) * sizeof(double) <= TL_LDS_LIMIT;
    wrong += fits != tl_applicable(Kc, 1024);
    if (Kc > 1) flips += fits != (tl_lds_doubles(Kc - 2, TS, ldx_max) * sizeof(double) <= TL_LDS_LIMIT);
  }
  wrong += flips != 1;
  // the slot lists and the kept centre frequencies hold every slot of a frame of 13 tile rows (n <= 51)
  wrong += !(TL_NSLOT > 51 && (4 * 51 + 18) / 16 == TL_NTMAX && (4 * 52 + 18) / 16 > TL_NTMAX);
  std::printf("%d wrong\n", wrong);
  return wrong != 0;
}
"""


def tile_rows(ncol):
    return (4 * np.asarray(ncol) + 18) >> 4


def frame_class(ncol):
    """LsArgs::cls: 0 for <= 8 tile rows, then one class per tile-row count up to 13."""
    return np.maximum(tile_rows(ncol) - 8, 0)


def wrap(d):
    return (d + np.pi) % (2 * np.pi) - np.pi


def state(name):
    """The engine of an input with adaptation 0 done and adaptation 1 prepared (tracks, slot lists)."""
    if name not in _cache:
        import torch
        assert torch.cuda.is_available(), "these tests need the MI355X"
        from eaqhm_amd.engine import DeviceAnalysis
        from test_gpu_tile_gather import _input
        from test_gpu_tile_threeweight_large import glide_signal, plan_for
        if name == "W":
            s, track = glide_signal(22400, wobble=1.2)
            plan = plan_for(s, track, 3)
        else:
            s, plan = _input(name)
        eng = DeviceAnalysis(s, s, plan, 70, 1, keep_raw=True)
        it = eng.adaptations()
        next(it)
        next(it)
        torch.cuda.synchronize()
        assert eng.ctx.ls_faults() == (0, 0, 0)
        _cache[name] = (eng, plan, eng.ncol.cpu().numpy()[:eng.nf].copy())
    return _cache[name]


def launch(name, sel, variant, tag=None):
    """eaqhm_ls_batch (adaptation 1) on frames `sel` of the input, in that order: frame i of the launch writes row i."""
    key = (name, tag, variant)
    if tag is not None and key in _cache:
        return _cache[key]
    import torch
    eng, p, _ = state(name)
    K, dev, nf = p.Kmax, eng.s.device, len(sel)
    idx = torch.as_tensor(np.asarray(sel), device=dev)
    tabs = [t[:eng.nf][idx].contiguous() for t in (eng.frame_c, eng.frame_wl, eng.frame_f0, eng.frame_K, eng.ncol)]
    cols = eng.cols.view(-1, K)[idx].contiguous().view(-1)
    inst = torch.arange(nf, dtype=torch.int32, device=dev)
    rec = torch.full((nf + 1, 3 * K + 1), float("nan"), dtype=torch.float64, device=dev)
    raw = [torch.full((nf, 2 * (2 * K + 1)), float("nan"), dtype=torch.float64, device=dev) for _ in range(2)]
    eng.ctx.set_option(1, variant)
    try:
        eng.ctx.ls_batch(1, eng.s, p.L, p.fs, eng.am_cur, eng.fm_cur, eng.track_t0, eng.track_len, K, inst, tabs[0], tabs[1],
                         tabs[2], tabs[3], tabs[4], cols, eng.seeded, eng.any_seed, nf, p.wl_max, 1, p.f0_stale, eng.f0min,
                         rec, raw[0], raw[1])
        torch.cuda.synchronize()
        faults = eng.ctx.ls_faults()
    finally:
        eng.ctx.set_option(1, 3)
    cx = lambda t: np.ascontiguousarray(t.cpu().numpy()).view(np.complex128)
    out = dict(records=rec.cpu().numpy(), amp=cx(raw[0]), slope=cx(raw[1]), faults=faults)
    if tag is not None:
        _cache[key] = out
    return out


def assert_values(tile, big, ncol, K):
    """Launch `tile` against launch `big` of the same frames."""
    assert tile["faults"] == (0, 0, 0) and big["faults"] == (0, 0, 0)
    worst = [0.0, 0.0]
    for f, n in enumerate(ncol):
        k = 2 * int(n) + 1
        for j, (key, tol) in enumerate((("amp", TOL_AMP), ("slope", TOL_SLOPE))):
            a, b = tile[key][f][:k], big[key][f][:k]
            e = np.abs(a - b).max() / np.abs(b).max()
            worst[j] = max(worst[j], e)
            assert np.isfinite(e) and e < tol, (key, f, int(n), e)
            assert np.isnan(tile[key][f][k:]).all()
    print("worst relative error of the raw amplitudes %.2e, of the raw slopes %.2e" % tuple(worst))
    nf = len(ncol)
    g, r = tile["records"][:nf], big["records"][:nf]
    assert np.isfinite(g).all() and np.isfinite(r).all()
    assert np.isnan(tile["records"][nf]).all()
    mg, mr = g[:, :K] != 0, r[:, :K] != 0
    assert np.mean(mg == mr) >= 0.999
    assert not (g[:, K:3 * K] != 0)[~np.tile(mg, 2)].any()
    both, top = mg & mr, r[:, :K].max()
    strong = both & (r[:, :K] > 1e-6 * top)
    worst = (np.abs(g[:, :K] - r[:, :K])[both].max() / top, np.abs(g[:, K:2 * K] - r[:, K:2 * K])[both].max(),
             np.abs(wrap(g[:, 2 * K:3 * K] - r[:, 2 * K:3 * K]))[strong].max(), np.abs(g[:, 3 * K] - r[:, 3 * K]).max() / top)
    print("record rows: amplitudes %.2e (relative), frequencies %.2e Hz, phases %.2e rad, DC %.2e (relative)" % worst)
    assert worst[0] <= TOL_AM_REL and worst[1] <= TOL_FM_HZ and worst[2] <= TOL_PH_RAD and worst[3] <= TOL_AM_REL


def assert_same_bits(a, b):
    for key in ("records", "amp", "slope"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


# ------------------------------------------------------------------------------------------------ values
@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_every_frame_against_the_large_frame_kernel(name):
    eng, plan, ncol = state(name)
    assert len(ncol) == plan.n_frames == 1430
    sel = np.arange(len(ncol))
    assert_values(launch(name, sel, 3, "all"), launch(name, sel, 2, "all"), ncol, plan.Kmax)


@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_same_launch_twice_same_bits(name):
    _, _, ncol = state(name)
    sel = np.arange(len(ncol))
    assert_same_bits(launch(name, sel, 3, "all"), launch(name, sel, 3, "again"))


# ------------------------------------------------------------------------------------------------ hand-out
def _batches(ncol, grid):
    """name -> frames of input A (indices, repeated where a class has too few)."""
    cl = frame_class(ncol)
    by = {c: np.flatnonzero(cl == c) for c in range(5)}
    assert all(len(v) >= 23 for v in by.values()), {c: len(v) for c, v in by.items()}     # A has classes 0..4
    rep = lambda c, m: by[c][np.arange(m) % len(by[c])]
    return {
        "one frame": by[2][:1],
        "one frame in each class": np.array([by[c][0] for c in range(5)]),
        "an empty class between two": np.concatenate((by[4][:3], by[2][:2], by[0][:4])),      # none of classes 3 and 1
        "fewer frames than compute units": np.concatenate([by[c][:7] for c in range(5)]),
        "grid frames of one class": rep(0, grid),
        "grid + 1 frames of one class": rep(3, grid + 1),
        "2 grid - 1 frames of one class": rep(1, 2 * grid - 1),
    }


BATCHES = ("one frame", "one frame in each class", "an empty class between two", "fewer frames than compute units",
           "grid frames of one class", "grid + 1 frames of one class", "2 grid - 1 frames of one class")


@gpu
@pytest.mark.parametrize("batch", BATCHES)
def test_every_frame_is_handed_out_exactly_once(batch):
    eng, plan, ncol = state("A")
    grid = eng.ctx.n_cu
    sel = _batches(ncol, grid)[batch]
    if batch == "fewer frames than compute units":
        assert len(sel) < grid
    full = launch("A", np.arange(len(ncol)), 3, "all")
    got = launch("A", sel, 3)
    assert got["faults"] == (0, 0, 0)
    done = ~np.isnan(got["records"]).all(axis=1)
    assert np.array_equal(np.flatnonzero(done), np.arange(len(sel))), (batch, np.flatnonzero(~done[:len(sel)])[:8])
    assert np.isfinite(got["records"][:len(sel)]).all()
    # each row is the row of ITS frame, to the bit: no frame done in place of another, none twice with another's slots
    assert np.array_equal(got["records"][:len(sel)], full["records"][sel])
    assert np.array_equal(got["amp"], full["amp"][sel], equal_nan=True)
    assert np.array_equal(got["slope"], full["slope"][sel], equal_nan=True)


# ------------------------------------------------------------------------------------------------ paths
@gpu
def test_bridged_slots():
    from test_gpu_tile_threeweight_large import gappy_frames
    eng, plan, ncol = state("W")
    gap = gappy_frames(eng.fm_cur.cpu().numpy(), int(eng.track_t0), plan)
    assert gap.sum() >= 16, int(gap.sum())
    sel = np.arange(len(ncol))
    tile, big = launch("W", sel, 3), launch("W", sel, 2)
    assert_values(tile, big, ncol, plan.Kmax)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from eaqhm_amd.hip import Context
    c = Context(0)
    yield c
    c.set_option(1, 3)


def _records_close(case, a, b):
    K, rows = case["Kmax"], case["frame_inst"][:case["n_frames"] - case["dropped"]]
    g, r = a["records"][rows], b["records"][rows]
    assert np.isfinite(g).all() and np.isfinite(r).all()
    mg, mr = g[:, :K] != 0, r[:, :K] != 0
    assert np.array_equal(mg, mr)
    top = r[:, :K].max()
    assert np.abs(g[:, :K] - r[:, :K]).max() <= TOL_AM_REL * top
    assert np.abs(g[:, K:2 * K] - r[:, K:2 * K]).max() <= TOL_FM_HZ
    return g, mg


@gpu
@pytest.mark.parametrize("name", ["G", "E"])
def test_gap_and_seed_sets_against_the_large_frame_kernel(ctx, name):
    """G: every branch of the gap bridging.  E: any_seed set (small frames: the flag reaches tile_frame through the header;
    the record of these classes reads the centre frequency through track_fm) — a seeded slot 0 shows 140 Hz."""
    case = R.BUILDERS[name]()
    ctx.set_option(1, 3)
    tile = R.run(case, ctx)
    ctx.set_option(1, 2)
    big = R.run(case, ctx)
    ctx.set_option(1, 3)
    assert tile["faults"] == big["faults"] and tile["faults"][:2] == (0, 0)
    g, mg = _records_close(case, tile, big)
    if name == "E":
        K = case["Kmax"]
        assert len(tile["seeded"]) > 0
        seeded = np.array([t["seeded"] for t in case["tags"]])
        assert seeded.any() and mg[seeded, 0].all()
        # 140 Hz + eta, not 0 + eta: an accepted slot has |eta| < f0_stale / 2 = 100 Hz, so the former lies above 40 Hz
        # whatever eta is (the model gives 93 .. 149 Hz here, i.e. eta = -47 .. 9 Hz: the latter would lie below 10 Hz)
        assert (g[seeded, K] > 40.0).all(), g[seeded, K]
    else:
        assert {t["gap"] for t in case["tags"]} == set(R.GAP_KINDS)


SEED_N = (40, 41, 42, 43)          # 11 tile rows each: the 9-slot budget (REC_ROW in tile_frame)


def case_seed11(seed=21):
    """Six frames, 3 samples apart, on each of four segments with n = 40 .. 43 active slots (slot 0 among them)."""
    fs, Kmax = 16000, 56
    b = R._Builder(fs, Kmax, seed)
    b.silence(16)
    for n in SEED_N:
        slots = np.arange(n)
        f0 = R._f0_for(slots, fs)                            # 7600 / n = 190 .. 176.7 Hz: slot 0 lies 37 .. 50 Hz above 140 Hz
        wl = R._wl(fs, f0)
        st = b.segment(2 * wl + 1 + 3 * 6 + 8, slots, f0)
        for i in range(6):
            b.frame(st + 2 + wl + 3 * i, wl, at_centre=(i == 2), before_centre=(i > 2))
    return b.finish("seed11", sort=False)


class SeedTheseCentres:
    """A backend (the context or the NumPy model) whose frame_prep also marks the given samples as seeded: eaqhm_ls_batch
    takes `seeded` / `any_seed` as inputs, and a frame centre that is seeded while slot 0 is active there is the input on
    which the kept centre frequency (the track's) and the one the record has to use (140 Hz) differ."""

    def __init__(self, be, centres):
        self._be, self._centres = be, [int(c) for c in centres]

    def __getattr__(self, name):
        return getattr(self._be, name)

    def frame_prep(self, *args):
        self._be.frame_prep(*args)
        seeded, any_seed = args[-2], args[-1]
        seeded[self._centres] = 1
        any_seed.fill_(1)

    def ls_faults(self):
        return self._be.ls_faults() if hasattr(self._be, "ls_faults") else None


@gpu
def test_seeded_slot_0_at_11_tile_rows_does_not_take_the_kept_frequency(ctx):
    from fake_backend import OracleBackend
    case = case_seed11()
    K, tags = case["Kmax"], case["tags"]
    assert [t["n"] for t in tags] == [n for n in SEED_N for _ in range(6)] and {t["nt"] for t in tags} == {11}
    at = np.array([t["at_centre"] for t in tags])
    centres = case["frame_c"][at]
    track0 = case["fm_full"][0, centres]
    assert (track0 > 140.0 + 33.0).all(), track0               # what a kept value would put in place of 140 Hz
    with R.one_thread():
        model = R.run(case, SeedTheseCentres(OracleBackend(), centres))
    # more frames than workgroups, so that frames arrive through the header too (frames of one source write the same row)
    src = np.arange(2 * ctx.n_cu + 24) % case["n_frames"]
    big_case = R.reorder(case, src)
    got = {}
    for variant in (3, 2):
        ctx.set_option(1, variant)
        got[variant] = R.run(big_case, SeedTheseCentres(ctx, centres))
    ctx.set_option(1, 3)
    tile, big = got[3], got[2]
    assert tile["faults"] == (0, 0, 0) and big["faults"] == (0, 0, 0)
    assert sorted(tile["seeded"].tolist()) == sorted(int(c) for c in centres)
    g, mg = _records_close(case, tile, big)                    # the large-frame kernel always goes through track_fm
    m = model["records"][case["frame_inst"]]
    assert mg[at, 0].all() and (m[at, 0] != 0).all()           # slot 0 is accepted in the frames seeded at the centre
    print("slot 0, frames seeded at the centre: record", g[at, K], "model", m[at, K], "track", track0)
    # 140 Hz + eta.  The model solves with inv(), the kernel by Cholesky: their eta agree far better than 1 Hz, and the
    # kept track value would be at least 33 Hz off
    assert (np.abs(g[at, K] - m[at, K]) < 1.0).all()
    assert (np.abs(g[at, K] - 140.0) < np.abs(g[at, K] - track0)).all()
    seen = np.array([t["before_centre"] for t in tags])       # the seed lies before the centre: slot 0 bridged, own value
    assert (np.abs(g[seen, K] - m[seen, K])[mg[seen, 0]] < 1.0).all()


@gpu
def test_mode_0_through_this_kernel_equals_the_resident_kernel(ctx):
    from test_gpu_a0_resident import KS, assert_same_bits as same, launch as launch_a0
    case = R._case_Z("ZR", 16000, 51, KS, 12)
    new, old = launch_a0(ctx, case, 1), launch_a0(ctx, case, 0)
    assert new["solved"] == case["n_frames"] and old["solved"] == 0
    assert new["faults"] == (0, 0, 0) and old["faults"] == (0, 0, 0)
    same(new, old)
    assert np.isfinite(old["records"][case["frame_inst"]]).all()


# ------------------------------------------------------------------------------------------------ host
def test_lds_budget_with_the_header(tmp_path):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert cxx, "no C++ compiler"
    exe, src = str(tmp_path / "tile_lds_check"), tmp_path / "tile_lds_check.cpp"
    src.write_text(LDS_CHECK)
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, "-o", exe, str(src)], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("\n0 wrong"), r.stdout[-2000:]
