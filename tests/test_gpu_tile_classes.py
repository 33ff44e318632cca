"""Raw LS solutions of eaqhm_ls_tile_kernel on every frame of an adaptation, size class by size class (tile rows of the
stacked system), against eaqhm_ls_mfma_kernel — the other batched kernel, whose Gramian is contracted separately and
whose raw solutions test_gpu_parity.py holds to the reference.  The classes use different Gramian forms (stacked tiles
or the three-weight Gramian over the basis); every class that has frames in the input is checked, at the raw-solution
tolerances of test_gpu_parity.py."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

TOL_AMP, TOL_SLOPE = 1e-9, 1e-8


def _plan_for(s, fs, track):
    from eaqhm_amd import prologue
    from eaqhm_amd.engine import FramePlan
    grid = prologue.resample_track(track, np.arange(0, len(s) - 1, round(fs * 5 / 1000)) / fs)
    frames, fstep = prologue.voiced_unvoiced_frames(s, fs, "female")
    prologue.apply_full_waveform(frames, len(s), 32 * 15)
    return FramePlan(len(s), fs, grid, frames, fstep, 15, 3, 32, 0)


def _raw_adaptation1(s, fs, track, variant):
    from eaqhm_amd.engine import DeviceAnalysis
    plan = _plan_for(s, fs, track)
    eng = DeviceAnalysis(s, s, plan, 160, 1, keep_raw=True)
    eng.ctx.set_option(1, variant)
    out = {}

    def hook(a, e):
        if a == 1:
            out["amp"] = e.raw[0].cpu().numpy().view(np.complex128).copy()
            out["slope"] = e.raw[1].cpu().numpy().view(np.complex128).copy()
            out["ncol"] = e.ncol.cpu().numpy()[:e.nf].copy()

    eng.run(on_adaptation=hook)
    return out


def _check_every_class(s, fs, track, need):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    tile, big = _raw_adaptation1(s, fs, track, 3), _raw_adaptation1(s, fs, track, 2)
    ncol = tile["ncol"]
    assert np.array_equal(ncol, big["ncol"])
    Kc = 2 * ncol + 1
    nt = (2 * Kc + 1 + 15) // 16
    seen = set()
    for c in range(1, 14):
        sel = np.flatnonzero(nt == c)
        if len(sel) == 0:
            continue
        seen.add(c)
        for f in sel:
            k = Kc[f]
            a, b = tile["amp"][f][:k], big["amp"][f][:k]
            sa, sb = tile["slope"][f][:k], big["slope"][f][:k]
            ea = np.abs(a - b).max() / np.abs(b).max()
            es = np.abs(sa - sb).max() / np.abs(sb).max()
            assert ea < TOL_AMP and es < TOL_SLOPE, (c, int(f), ea, es)
    assert need <= seen, sorted(seen)


def test_tile_classes_sa19():
    from eaqhm_amd import prologue
    g = load_golden("sa19_female_default.npz")
    fs, s = prologue.read_signal(os.path.join(GOLDEN, "SA19.WAV"))
    _check_every_class(s, fs, g["swipe_track"], {8, 9, 10})


def test_tile_classes_synth16k():
    """The first 4 s of bench.py's synth16k_60s workload (signal and pitch track)."""
    from eaqhm_amd.synth import synth_speech_int16
    fs = 16000
    s = synth_speech_int16(60.0, fs)[:4 * fs] / 32768.0
    track = load_golden("prep_fixtures.npz")["synth16k_60s_f0s_5ms"]
    _check_every_class(s, fs, track[track[:, 0] < 4.0], {8, 9, 10, 11, 12})
