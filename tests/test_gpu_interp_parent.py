"""eaqhm_spline_kernel and eaqhm_eval_kernel on the MI355X against the outputs of the commit before their blocks moved
onto the knot grid and their record rows into LDS: sha256 digests of every case of tests/interp_parent_cases.py,
recorded on the MI355X at the commit tests/golden/interp_parent_digests.json names.  And, independent of the fixture,
what a grid fixed to the knots can get wrong: every start offset of a range against the whole run (first and last
partial block, a range inside one block, a short range across a block boundary), the limbs of uneven pieces, and
sub-range spline solves.  Everything here is compared bit for bit."""
import json

import numpy as np
import pytest

import interp_parent_cases as P
import interp_stage_ref as R
from test_gpu_interp_stage import SENTINEL, Stage, cuts_of

pytestmark = pytest.mark.gpu

SMALL = [c["name"] for c in P.GEOMETRY]
OFFSETS = range(0, 131)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from eaqhm_amd.functions import _ctx
    return _ctx(0)


_STAGE = {}


def stage(ctx, name):
    """(Stage, its whole-range outputs) — computed once per case."""
    if name not in _STAGE:
        case = next(c for c in P.all_cases() if c["name"] == name)
        st = Stage(ctx, case)
        _STAGE[name] = (st, P.outputs(st), st.evaluate())
    return _STAGE[name]


def test_every_case_is_the_parents_bit_for_bit(ctx):
    with open(P.FIXTURE) as f:
        want = json.load(f)["cases"]
    names = [c["name"] for c in P.all_cases()]
    assert set(names) == set(want) and len(names) == 11 + 2 * len(P.STEPS) + 1
    bad = []
    for name in names:
        out = stage(ctx, name)[1]
        assert set(out) == set(want[name])
        bad += ["%s.%s" % (name, key) for key in sorted(out) if P.digest(out[key]) != want[name][key]]
    assert not bad, bad


def check_range(st, whole, lo, hi, synth):
    part = st.evaluate(lo, hi, pad=(3, 4), synth=synth)
    t0 = part["t0"]
    for key in ("am", "fm"):
        assert np.array_equal(part[key][:, lo - t0:hi - t0], whole[key][:, lo:hi]), (key, lo, hi)
        assert np.all(part[key][:, :lo - t0] == SENTINEL) and np.all(part[key][:, hi - t0:] == SENTINEL), (key, lo, hi)
    if not synth:
        return
    assert np.array_equal(part["s_hat"][lo:hi], whole["s_hat"][lo:hi]), (lo, hi)
    assert np.all(part["s_hat"][:lo] == SENTINEL) and np.all(part["s_hat"][hi:] == SENTINEL), (lo, hi)
    inst = np.arange(st.T) * st.D
    inside = (inst >= lo) & (inst < hi)
    assert np.array_equal(part["ph_knot"][inside], whole["ph_knot"][inside]), (lo, hi)
    assert np.all(part["ph_knot"][~inside] == SENTINEL), (lo, hi)


@pytest.mark.parametrize("name", SMALL)
def test_every_offset_gives_the_whole_runs_slice(ctx, name):
    st, _, whole = stage(ctx, name)
    L = st.L
    n = 0
    for o in OFFSETS:
        lo, hi = o, L - (o % 7)
        if lo >= hi:
            continue
        check_range(st, whole, lo, hi, synth=True)
        n += 1
    assert n >= min(len(OFFSETS), L - 6)
    # short ranges across the boundaries of every block size in use (multiples of 16 / 30 / 32 / 45 / 60 / 64 and of
    # the step), and a range inside one block
    for c in sorted({16, 30, 32, 45, 60, 64, st.D, 2 * st.D, 4 * st.D}):
        for lo, hi in ((c - 7, c + 8), (c - 1, c + 1), (c, c + 1), (c + 1, c + 9)):
            if 0 <= lo < hi <= L:
                check_range(st, whole, lo, hi, synth=True)
    # track-only passes (s_hat NULL): an odd offset, a start on a block boundary, fewer than 16 samples across one
    o = 37 % max(L - 8, 1)
    check_range(st, whole, o, L - (o % 7), synth=False)
    for c in (45, 3 * st.D, 64):
        for lo, hi in ((c, L), (c - 5, c + 6)):
            if 0 <= lo < hi <= L:
                check_range(st, whole, lo, hi, synth=False)


@pytest.mark.parametrize("name", SMALL)
def test_limbs_of_uneven_pieces_add_up(ctx, name):
    st, out, _ = stage(ctx, name)
    cuts = cuts_of(st.L, st.D, (0.29, 0.64))
    if len(cuts) < 4:                                           # (a signal of a few dozen samples: two pieces)
        cuts = [0, max(1, st.L // 3), st.L]
    total = [0] * 8
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = st.evaluate(lo, hi)
        assert part["limbs"][7] == int(out["limbs"][7])
        total = [a + b for a, b in zip(total, part["limbs"][:7] + [0])]
    assert R.ints_of(total)[:3] == R.ints_of(out["limbs"])[:3], (cuts, total, out["limbs"])


# the 300-instant case: ten instant tiles, runs longer than 80 knots (the weight table), tile seams inside sub-ranges
@pytest.mark.parametrize("name", SMALL + ["b32_s15_k59_16k"])
def test_subrange_solves_give_the_whole_solve(ctx, name):
    st, out, _ = stage(ctx, name)
    T = st.T
    wins = [(i_lo, T - (i_lo % 3)) for i_lo in range(0, 9)]
    if T > 250:
        wins += [(100, 171), (57, 250), (133, 134)]
    for i_lo, i_hi in wins:
        code, mom = st.solve(i_lo, i_hi)
        code, mom = code.cpu().numpy(), mom.cpu().numpy()
        assert np.array_equal(code[i_lo:i_hi], out["code"][i_lo:i_hi]), (i_lo, i_hi)
        assert np.array_equal(mom[i_lo:i_hi], out["mom"][i_lo:i_hi]), (i_lo, i_hi)
        assert np.array_equal(code[:4], out["code"][:4]), (i_lo, i_hi)
        # written: the range, two instants either side (the end conditions' neighbours) and rows 0..3
        outside = np.ones(T, bool)
        outside[max(i_lo - 2, 0):min(i_hi + 2, T)] = False
        outside[:4] = False
        assert np.all(code[outside] == 99) and np.all(mom[outside] == SENTINEL), (i_lo, i_hi)
