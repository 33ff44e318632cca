"""eaqhm_ls_batch called directly, every frame of both batched kernels held to the NumPy model.

The cases come from tests/ls_batch_ref.py (sets S, G, P, P0, E, Z16, Z48, B: every system size, every branch of the gap
bridging, every placement of a window against the resident tracks and the 1024-sample zero-count chunks, empty-row
seeding, adaptation 0, large frames only); tests/test_ls_batch_cases_cpu.py asserts without a GPU that they hold what
they promise and that every frame is conditioned well enough for the bars used here to mean something (three CPU solves
of the same normal equations agree to 1/10 of them).  The reference is tests/fake_backend.py, OracleBackend.ls_batch.

Which kernels the frames go through.  With EAQHM_OPT_LS_VARIANT = 3 a launch takes the tile path when
ls_tile_applicable(Kcmax, Nmax) holds: Nmax = 2 wl_max + 1 <= 64 * CI_NCH = 1024, and
    tl_lds_doubles = max(tl_usize_c, tl_usize_g) + 4 Kcmax + 16 + 2 * 64 * CI_NCH + 16 * TL_NTMAX
                   = max(16224, 16240) + 4 Kcmax + 16 + 2048 + 208 = 18512 + 4 Kcmax doubles <= 159 KiB = 20352 doubles,
i.e. Kcmax <= 460, Kmax <= 229.  S, G, P, P0, E (Kmax = 56, N <= 1023) and Z16 (Kmax = 60: frame_K = 60 needs it;
N <= 423) are inside it: frames of up to 13 tile rows (n <= 51) run in eaqhm_ls_tile_kernel (tile_frame, adaptation 0:
a0_frame), the larger ones (n = 52, 54, 56; frame_K = 52, 60) are left to the second launch — eaqhm_ls_mfma_kernel,
adaptation 0: eaqhm_ls_a0big_kernel.  B (wl_max = 560, N = 1121) and Z48 (wl_max = 571) are outside it: every frame
goes through launch_ls_mfma with min_nb = 0, as every frame of every set does with variant 2 — mode 1 in
eaqhm_ls_mfma_kernel, mode 0 in eaqhm_ls_a0big_kernel up to MF_A0_M = 19 real tile rows (frame_K <= 151) and in the
mode-0 branch of eaqhm_ls_mfma_kernel beyond (frame_K = 152, 170).

Bars (tests/test_gpu_parity.py): raw amplitudes within 1e-9 of the frame's largest reference amplitude, raw slopes
within 1e-8 of its largest slope, for EVERY frame; record rows at TOL_AM_REL / TOL_FM_HZ / TOL_PH_RAD."""
import time

import numpy as np
import pytest

import ls_batch_ref as R
from conftest import record_measurement

pytestmark = pytest.mark.gpu

TOL_AM_REL, TOL_FM_HZ, TOL_PH_RAD = 1e-8, 1e-3, 1e-5      # tests/test_gpu_parity.py
BAR_AMP, BAR_SLOPE = 1e-9, 1e-8
SETS = ("S", "G", "P", "P0", "E", "Z16", "Z48", "B")
VARIANTS = (3, 2)


def wrap(d):
    return (d + np.pi) % (2 * np.pi) - np.pi


@pytest.fixture(scope="module")
def reference():
    """name -> (case, model result, per-frame inv()-to-Cholesky distance of the reference's own numbers), each computed
    once and never changed."""
    cache = {}

    def get(name):
        if name not in cache:
            from scipy.linalg import cho_factor, cho_solve
            case = R.BUILDERS[name]()
            with R.one_thread():
                ref = R.run(case)
                dist = np.zeros((case["n_frames"] - case["dropped"], 2))
                for f, Ew, ws in R.systems(case, ref):
                    EwH = Ew.conj().T
                    Rm, rhs = EwH @ Ew, EwH @ ws
                    Kc = len(rhs) // 2
                    d = np.abs(cho_solve(cho_factor(Rm), rhs) - np.linalg.inv(Rm) @ rhs)
                    dist[f] = (d[:Kc].max() / np.abs(ref["raw_amp"][f, :Kc]).max(),
                               d[Kc:].max() / np.abs(ref["raw_slope"][f, :Kc]).max())
            cache[name] = (case, ref, dist)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from eaqhm_amd.hip import Context
    c = Context(0)
    yield c
    c.set_option(1, 3)


@pytest.fixture(scope="module")
def launched(ctx, reference):
    """(set, variant) -> result of ONE launch of the set as built (for S: ascending n), shared by the tests."""
    cache = {}

    def get(name, variant):
        if (name, variant) not in cache:
            ctx.set_option(1, variant)
            assert ctx.ls_faults() == (0, 0, 0)
            t0 = time.perf_counter()
            got = R.run(reference(name)[0], ctx)
            got["seconds"] = time.perf_counter() - t0
            cache[name, variant] = got
        return cache[name, variant]
    return get


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", SETS)
def test_every_frame_against_the_model(reference, launched, name, variant):
    case, ref, dist = reference(name)
    got = launched(name, variant)
    K, nf, tags = case["Kmax"], case["n_frames"], case["tags"]
    live = nf - case["dropped"]
    # the one frame of set P whose window starts before the resident tracks is dropped and counted, nothing else is
    assert got["faults"] == (0, 0, case["dropped"])

    # ---- raw solutions: every frame
    err = R.frame_errors(got, ref, case)
    per_nt = {}
    for f in range(live):
        w = per_nt.setdefault(tags[f]["nt"], np.zeros(4))
        w[:] = np.maximum(w, (err[f, 0], err[f, 1], dist[f, 0], dist[f, 1]))
    record_measurement("ls_direct_%s_v%d" % (name, variant), frames=live, launch_seconds=round(got["seconds"], 4),
                       worst_amp_over_bar=float(err[:, 0].max() / BAR_AMP), worst_slope_over_bar=float(err[:, 1].max() / BAR_SLOPE),
                       per_tile_rows={str(nt): dict(amp=w[0], slope=w[1], ref_inv_vs_cholesky_amp=w[2],
                                                    ref_inv_vs_cholesky_slope=w[3]) for nt, w in sorted(per_nt.items())})
    print("%s v%d: worst amplitude %.2e, slope %.2e (reference's inv-Cholesky %.1e / %.1e)"
          % (name, variant, err[:, 0].max(), err[:, 1].max(), dist[:, 0].max(), dist[:, 1].max()))
    bad = ["%s v%d nt=%d n=%d wl=%d gap=%s: amplitudes %.2e, slopes %.2e"
           % (name, variant, tags[f]["nt"], tags[f]["n"], tags[f]["wl"], tags[f]["gap"], err[f, 0], err[f, 1])
           for f in range(live) if not (err[f, 0] <= BAR_AMP and err[f, 1] <= BAR_SLOPE)]
    assert not bad, "%d frames off the bars:\n%s" % (len(bad), "\n".join(bad[:30]))
    for f in range(nf):                                     # nothing written past a frame's Kc columns, nor for a dropped frame
        Kc = 2 * tags[f]["n"] + 1 if f < live else 0
        assert np.isnan(got["raw_amp"][f, Kc:]).all() and np.isnan(got["raw_slope"][f, Kc:]).all(), f

    # ---- record rows
    rows = case["frame_inst"][:live]
    g, r = got["records"], ref["records"]
    assert np.isfinite(g[rows]).all()                       # a frame rewrites its whole row of 3 Kmax + 1 entries
    others = np.setdiff1d(np.arange(case["n_rows"]), rows)
    assert len(others) == 3 + case["dropped"] and np.isnan(g[others]).all()   # every other row keeps the sentinel
    g, r = g[rows], r[rows]
    assert np.isfinite(r).all()
    mg, mr = g[:, :K] != 0, r[:, :K] != 0
    assert np.mean(mg == mr) >= 0.999
    assert not (g[:, K:3 * K] != 0)[~np.tile(mg, 2)].any()          # frequency and phase only where accepted
    both = mg & mr
    top = r[:, :K].max()
    assert np.abs(g[:, :K] - r[:, :K])[both].max() <= TOL_AM_REL * top
    assert np.abs(g[:, K:2 * K] - r[:, K:2 * K])[both].max() <= TOL_FM_HZ
    strong = both & (r[:, :K] > 1e-6 * top)
    assert np.abs(wrap(g[:, 2 * K:3 * K] - r[:, 2 * K:3 * K]))[strong].max() <= TOL_PH_RAD
    assert np.abs(g[:, 3 * K] - r[:, 3 * K]).max() <= TOL_AM_REL * top       # the DC entry


def _same_bits(case, a, b, order):
    """Launch `a` ran the frames `order` of the case, launch `b` all of them as built: rows and raw solutions of those
    frames, bit for bit."""
    rows = case["frame_inst"][order]
    assert np.array_equal(a["records"][rows], b["records"][rows])
    assert np.isfinite(a["records"][rows]).all()
    for key in ("raw_amp", "raw_slope"):
        assert np.array_equal(a[key], b[key][order], equal_nan=True), key


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("order", ["descending", "shuffled"])
def test_queue_order_does_not_change_a_bit(ctx, reference, launched, order, variant):
    """The workgroups reuse LDS planes and scratch between frames of different sizes: a frame's row and raw solution do
    not depend on which frames ran before it on the same workgroup."""
    case = reference("S")[0]
    base = launched("S", variant)                          # ascending n
    nf = case["n_frames"]
    perm = np.arange(nf)[::-1] if order == "descending" else np.random.default_rng(11).permutation(nf)
    ctx.set_option(1, variant)
    got = R.run(R.reorder(case, perm), ctx)
    assert got["faults"] == (0, 0, 0)
    _same_bits(case, got, base, perm)


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_frame_alone_gives_the_same_bits(ctx, reference, launched, variant):
    case = reference("S")[0]
    base = launched("S", variant)
    ctx.set_option(1, variant)
    sizes = [t["n"] for t in case["tags"]]
    for n in R.SINGLES:
        f = sizes.index(n) + 5                             # one of the sixteen windows of that size
        assert sizes[f] == n
        got = R.run(R.reorder(case, [f]), ctx)
        assert got["faults"] == (0, 0, 0)
        _same_bits(case, got, base, np.array([f]))
        others = np.setdiff1d(np.arange(case["n_rows"]), case["frame_inst"][[f]])
        assert np.isnan(got["records"][others]).all()
