"""The classes of 11 and 12 tile rows of eaqhm_ls_tile_kernel contract the three-weight Gramian unit by unit
(csrc/eaqhm_ls_twunits.h: forms K3, K4 and, on the diagonal basis pairs, H).  Raw adaptation-1 solutions of the tile
kernel, frame by frame, against eaqhm_ls_mfma_kernel — as test_gpu_tile_classes.py does, at its tolerances — on inputs
made for these classes: every column count n = 40..47 (Kc = 81..95: both ends of each class, Kc + 1 = 82 and 88 with two
and eight live columns in the sixth basis tile column), slots whose window has gaps (their bridged rows lie in the
scratch area that the G_p tiles are written to afterwards), and windows whose last chunk of 16 sample pairs holds 1, 2,
15 and 16 pairs.

The inputs were chosen with oracle/eaqhm_oracle.py (Analysis.ls_stage(0) / post_stage(0), then the nonzero slots of
fm_current at every frame centre): the glide 163 -> 197.5 Hz gives n = 47 .. 40 at adaptation 1, the track with
alternating +-1.2 Hz on its 5 ms grid switches the top slot on and off every few frames near each step of n."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_AMP, TOL_SLOPE = 1e-9, 1e-8      # test_gpu_tile_classes.py
FS = 16000
LAST_CHUNK = {1, 2, 15, 0}           # (wl + 1) mod 16: sample pairs in the last chunk (0: a full one)


def glide_signal(n, f_lo=163.0, f_hi=197.5, wobble=0.0, seed=5):
    """Harmonic glide with a little noise (16-bit), and its f0 track at 1 ms; `wobble` adds alternating +- Hz to the
    track at the points of the 5 ms grid (the signal keeps the smooth glide)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    f0 = f_lo + (f_hi - f_lo) * t / t[-1]
    phi = 2 * np.pi * np.cumsum(f0) / FS
    x = np.zeros(n)
    for k in range(1, 49):
        x += k ** -1.1 * np.cos(k * phi + rng.uniform(0, 2 * np.pi)) * (k * f0 < 0.49 * FS)
    x += rng.standard_normal(n) * np.sqrt(np.mean(x ** 2)) * 10 ** (-50 / 20)
    s = np.round(0.25 * x / np.abs(x).max() * 32767) / 32768.0
    tt = np.arange(0, n / FS, 0.001)
    ft = f_lo + (f_hi - f_lo) * tt / t[-1]
    if wobble:
        ft = ft + wobble * np.where((np.round(tt / 0.005).astype(int) & 1) == 1, 1.0, -1.0)
    return s, np.column_stack([tt, ft, np.ones_like(tt)])


def plan_for(s, track, pitch_periods):
    from eaqhm_amd import prologue
    from eaqhm_amd.engine import FramePlan
    grid = prologue.resample_track(track, np.arange(0, len(s) - 1, round(FS * 5 / 1000)) / FS)
    frames, fstep = prologue.voiced_unvoiced_frames(s, FS, "other")
    for fr in frames:
        fr.isSpeech = fr.isVoiced = True
    return FramePlan(len(s), FS, grid, frames, fstep, 15, pitch_periods, 32, 0)


def _raw_adaptation1(s, plan, variant):
    from eaqhm_amd.engine import DeviceAnalysis
    eng = DeviceAnalysis(s, s, plan, 70, 1, keep_raw=True)
    eng.ctx.set_option(1, variant)
    out = {}

    def hook(a, e):
        if a == 0:      # the tracks that adaptation 1 reads
            out["fm"] = e.fm_cur.cpu().numpy().copy()
            out["t0"] = int(e.track_t0)
        if a == 1:
            out["amp"] = e.raw[0].cpu().numpy().view(np.complex128).copy()
            out["slope"] = e.raw[1].cpu().numpy().view(np.complex128).copy()
            out["ncol"] = e.ncol.cpu().numpy()[:e.nf].copy()

    eng.run(on_adaptation=hook)
    assert eng.ctx.ls_faults() == (0, 0, 0)
    return out


def gappy_frames(fm, t0, plan):
    """Frames with an active slot (nonzero at the centre) whose track has a zero inside the frame's window."""
    out = np.zeros(plan.n_frames, dtype=bool)
    for f in range(plan.n_frames):
        c, wl = int(plan.frame_c[f]) - t0, int(plan.frame_wl[f])
        w = fm[:, c - wl:c + wl + 1]
        out[f] = bool(((w == 0).any(axis=1) & (fm[:, c] != 0)).any())
    return out


def _compare(s, track, pitch_periods):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    plan = plan_for(s, track, pitch_periods)
    tile, big = _raw_adaptation1(s, plan, 3), _raw_adaptation1(s, plan, 2)
    ncol = tile["ncol"]
    assert len(ncol) == plan.n_frames and np.array_equal(ncol, big["ncol"])
    Kc = 2 * ncol + 1
    nt = (2 * Kc + 1 + 15) // 16
    worst = {}
    for f in np.flatnonzero((nt >= 10) & (nt <= 13)):
        k = Kc[f]
        a, b = tile["amp"][f][:k], big["amp"][f][:k]
        sa, sb = tile["slope"][f][:k], big["slope"][f][:k]
        ea = np.abs(a - b).max() / np.abs(b).max()
        es = np.abs(sa - sb).max() / np.abs(sb).max()
        w = worst.setdefault(int(nt[f]), [0.0, 0.0])
        w[0], w[1] = max(w[0], ea), max(w[1], es)
        assert ea < TOL_AMP and es < TOL_SLOPE, (int(nt[f]), int(f), int(ncol[f]), int(plan.frame_wl[f]), ea, es)
    print("worst relative error per class (amplitude, slope):", worst)
    return plan, ncol, nt, tile


def test_every_column_count_of_the_classes():
    """1.4 s glide, 3 pitch periods per window: n = 40..47, every one of them; the windows of this glide also end on every
    last-chunk shape in question (wl = 127, 128 at 11 tile rows, wl = 142, 143 at 12)."""
    s, track = glide_signal(22400)
    plan, ncol, nt, _ = _compare(s, track, 3)
    assert set(range(40, 48)) <= set(ncol.tolist()), sorted(set(ncol.tolist()))
    large = (nt == 11) | (nt == 12)
    assert LAST_CHUNK <= set(((plan.frame_wl[large] + 1) % 16).tolist())


def test_last_chunk_shapes_with_longer_windows():
    """The same column counts under windows of 4 pitch periods (wl = 164..196, 11-13 chunks): the windows of each of
    the two classes end on every one of the 16 last-chunk shapes, the four in question among them."""
    s, track = glide_signal(22400)
    plan, ncol, nt, _ = _compare(s, track, 4)
    for c in (11, 12):
        assert LAST_CHUNK <= set(((plan.frame_wl[nt == c] + 1) % 16).tolist()), c


def test_bridged_slots_in_the_classes():
    """The f0 track alternates by +-1.2 Hz on its 5 ms grid, so near each step of K = floor(7800 / f0) the top slot is
    there in some frames and missing in their neighbours: its track has gaps inside the windows that cover it."""
    s, track = glide_signal(22400, wobble=1.2)
    plan, ncol, nt, tile = _compare(s, track, 3)
    gap = gappy_frames(tile["fm"], tile["t0"], plan)
    assert (gap & (nt == 11)).sum() >= 8 and (gap & (nt == 12)).sum() >= 8, ((gap & (nt == 11)).sum(), (gap & (nt == 12)).sum())
