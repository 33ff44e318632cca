"""The continuous pitch track on the MI355X (eaqhm_amd.pitch -> eaqhm_viterbi_forward / _backtrack / _refine) against
tests/viterbi_ref.py, the NumPy model that tests/test_pitch_viterbi_cpu.py ties to an enumeration of all paths.

The recurrence has no product and every tie is decided by rule, so the path, the back-pointers, the tile maps and the
last column are EQUAL to the float64 model's: integers equal, doubles equal as bits.  The refinement has products: its
pitch (read from the host's table) is equal as bits wherever the fine-grid maximum is decided (swipe_ref.GAP), and its
strength is within swipe_ref.bar of the long-double model: 100 x the model's own float64-to-long-double difference, at
least 64 u (strengths are at most about 1)."""
import os
import re

import numpy as np
import pytest

import swipe_ref as R
import viterbi_ref as V
from conftest import GOLDEN, ROOT, record_measurement

pytestmark = pytest.mark.gpu

LD = np.longdouble
TILE = int(re.search(r"#define\s+EAQHM_VITERBI_TILE\s+(\d+)",
                     open(os.path.join(ROOT, "include", "eaqhm_viterbi.h")).read()).group(1))
CASES = V.cases(TILE)
NPCS = (3, 63, 64, 65, 273, 1024)                     # the grid of viterbi_ref.cases; its named cases have 5 and 7
SENTINEL = -12345


@pytest.fixture(scope="module")
def amd():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import eaqhm_amd
    return eaqhm_amd


def ctx():
    import torch
    from eaqhm_amd.functions import _ctx
    c = _ctx(0)
    return torch, c, c.device


def up(a):
    torch, _, d = ctx()
    return torch.as_tensor(np.ascontiguousarray(a), device=d)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 1. forward and backtrack
def gpu_decode(S, cost, unvoiced):
    """-> (bp, tilemap, last, q) with nothing written behind any of them."""
    torch, c, d = ctx()
    npc, T = S.shape
    ntiles = -(-T // TILE)
    bp = torch.full((T + 1, npc + 1), SENTINEL, dtype=torch.int16, device=d)
    tm = torch.full((ntiles + 1, npc + 1), SENTINEL, dtype=torch.int16, device=d)
    last = torch.full((npc + 1 + 4,), np.nan, dtype=torch.float64, device=d)
    q = torch.full((T + 4,), SENTINEL, dtype=torch.int32, device=d)
    c.viterbi_forward(up(S), npc, T, up(cost), len(cost) - 1, unvoiced, bp[:T], tm[:ntiles], last[:npc + 1])
    c.viterbi_backtrack(bp[:T], tm[:ntiles], last[:npc + 1], npc, T, q[:T])
    bp_h, tm_h, last_h, q_h = bp.cpu().numpy(), tm.cpu().numpy(), last.cpu().numpy(), q.cpu().numpy()
    assert (bp_h[T:] == SENTINEL).all() and (tm_h[ntiles:] == SENTINEL).all()
    assert np.isnan(last_h[npc + 1:]).all() and (q_h[T:] == SENTINEL).all()
    return bp_h[:T], tm_h[:ntiles], last_h[:npc + 1], q_h[:T]


@pytest.mark.parametrize("npc", NPCS)
def test_forward_and_backtrack(amd, npc):
    mine = [c for c in CASES if c[1].shape[0] == npc]
    assert {c[1].shape[1] for c in mine} >= {1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5}
    assert {len(c[2]) - 1 for c in mine} >= {0, 1, min(48, npc - 1), min(npc - 1, 256)}
    entered = left = 0
    for name, S, cost, unvoiced in mine:
        m = V.forward(S, cost, unvoiced, TILE)
        bp, tm, last, q = gpu_decode(S, cost, unvoiced)
        assert np.array_equal(q, m["q"]), name
        assert np.array_equal(bp, m["bp"]), name
        assert np.array_equal(tm, m["tilemap"]), name
        assert np.array_equal(bits(last), bits(m["last"])), name
        again = gpu_decode(S, cost, unvoiced)
        assert all(np.array_equal(a, b) for a, b in zip((bp, tm, q), again[:2] + again[3:])), name
        assert np.array_equal(bits(last), bits(again[2])), name
        assert q.min() >= 0 and q.max() <= npc - (unvoiced is None)
        assert np.abs(np.diff(q.astype(np.int64)))[(q[1:] < npc) & (q[:-1] < npc)].max(initial=0) <= len(cost) - 1
        if unvoiced is not None:
            entered += int((q == npc).any())
            left += int((q < npc).any())
    print("npc %d: %d cases, the unvoiced state on the path in %d, a voiced state in %d" % (npc, len(mine), entered, left))
    record_measurement("viterbi_forward_npc%d" % npc, cases=len(mine))
    if npc >= 63:
        assert entered and left


def test_unvoiced_state_paths(amd):
    """uv so low the state is never entered, so high it is never left, entered at t = 0, left at T - 1."""
    by = {c[0]: c for c in CASES}
    low = [c for c in CASES if c[3] is not None and c[3][0] == -64.0 and c[1].shape[1] > 1]
    high = [c for c in CASES if c[3] is not None and c[3][0] == 64.0 and c[1].shape[1] > 1]
    assert low and high
    for name, S, cost, unvoiced in low[:6]:
        assert (gpu_decode(S, cost, unvoiced)[3] < S.shape[0]).all(), name
    for name, S, cost, unvoiced in high[:6]:
        assert (gpu_decode(S, cost, unvoiced)[3] == S.shape[0]).all(), name
    _, S, cost, unvoiced = by["entered-at-0-left-at-end"]
    q = gpu_decode(S, cost, unvoiced)[3]
    assert q[0] == 5 and q[-2] == 5 and q[-1] == 2
    _, S, cost, unvoiced = by["left-after-0"]
    q = gpu_decode(S, cost, unvoiced)[3]
    assert q[0] == 5 and (q[1:] == 3).all()
    for name, S, cost, unvoiced in (c for c in CASES if c[1].shape[0] not in NPCS):   # the named cases against the model
        m = V.forward(S, cost, unvoiced, TILE)
        bp, tm, last, q = gpu_decode(S, cost, unvoiced)
        assert np.array_equal(q, m["q"]) and np.array_equal(bp, m["bp"]) and np.array_equal(tm, m["tilemap"]), name
        assert np.array_equal(bits(last), bits(m["last"])), name


# ---- 2. the refinement
def gpu_refine(S, q, pc, ntc, nftc, ptab, nf):
    torch, c, d = ctx()
    npc, T = S.shape
    p = torch.full((T + 4,), np.nan, dtype=torch.float64, device=d)
    s = torch.full((T + 4,), np.nan, dtype=torch.float64, device=d)
    c.viterbi_refine(up(S), up(q.astype(np.int32)), npc, T, up(pc), up(ntc), up(nftc), up(ptab), up(nf.astype(np.int32)),
                     nftc.shape[1], p[:T], s[:T])
    ph, sh = p.cpu().numpy(), s.cpu().numpy()
    assert np.isnan(ph[T:]).all() and np.isnan(sh[T:]).all()
    return ph[:T], sh[:T]


def check_refine(name, S, q, pc, ntc, nftc, ptab, nf):
    npc = S.shape[0]
    m64 = V.refine(S, q, pc, ntc, nftc, ptab, nf)
    mld = V.refine(S, q, pc, ntc, nftc, ptab, nf, LD)
    p, s = gpu_refine(S, q, pc, ntc, nftc, ptab, nf)
    p2, s2 = gpu_refine(S, q, pc, ntc, nftc, ptab, nf)
    assert np.array_equal(bits(p), bits(p2)) and np.array_equal(bits(s), bits(s2))
    dec = (mld["gap"] > R.GAP) & (m64["gap"] > R.GAP)
    bar = R.bar(np.abs(m64["s"] - mld["s"]).max())
    err = float(np.abs(s - mld["s"]).max())
    print("refine %s: %d of %d instants decided, s error / bar %.3g (bar %.2e)" % (name, dec.sum(), len(q), err / bar, bar))
    record_measurement("viterbi_refine_" + name, decided=int(dec.sum()), s_err_over_bar=err / bar)
    assert np.array_equal(bits(p[dec]), bits(mld["p"][dec]))
    assert err <= bar
    unv, edge = q >= npc, (q == 0) | (q == npc - 1)
    assert not p[unv].any() and not s[unv].any()
    assert np.array_equal(bits(p[edge]), bits(pc[q[edge]])) and np.array_equal(bits(s[edge]), bits(S[q[edge], edge.nonzero()[0]]))
    return p, s, dec


@pytest.mark.parametrize("T", (1, 255, 256, 257))
def test_refine_hand_made(amd, T):
    """Random scores and a path that visits every kind of state: inner, both edges, unvoiced."""
    rng = np.random.default_rng(T)
    npc, nfine = 70, 16
    S = rng.uniform(0.1, 1.0, (npc, T))
    q = rng.integers(1, npc - 1, T)
    q[::7], q[3::7], q[5::7] = 0, npc - 1, npc
    inner = np.flatnonzero((q > 0) & (q < npc - 1))
    S[q[inner], inner] += 1.0                                                # a peak on the path: the quadratic opens downwards
    ntc = np.tile(np.array([-0.125, 0.0, 0.125]), (npc, 1)) * rng.uniform(0.9, 1.1, (npc, 1))
    nftc = np.sort(rng.uniform(-0.12, 0.12, (npc, nfine)), axis=1)
    ptab = 100.0 + np.arange(npc)[:, None] + np.arange(nfine)[None, :] / 64.0
    nf = rng.integers(1, nfine + 1, npc)
    pc = 100.0 + np.arange(npc) + 0.5
    p, s, dec = check_refine("hand_T%d" % T, S, q, pc, ntc, nftc, ptab, nf)
    assert dec[inner].mean() > 0.9 if len(inner) > 10 else True
    assert np.all(np.isin(p, np.concatenate((ptab.ravel(), pc, [0.0]))))


def test_refine_even_quadratic_takes_the_first_point(amd):
    npc, T, nfine = 9, 3, 16
    S = np.full((npc, T), 1.0)
    S[4] = 2.0                                                               # equal neighbours, symmetric abscissae: c1 = 0
    ntc = np.tile(np.array([-0.125, 0.0, 0.125]), (npc, 1))
    nftc = np.tile((np.arange(nfine) - (nfine - 1) / 2) / 64.0, (npc, 1))
    ptab = 100.0 + np.arange(npc)[:, None] + np.arange(nfine)[None, :] / 64.0
    p, s = gpu_refine(S, np.full(T, 4), 50.0 + np.arange(npc), ntc, nftc, ptab, np.full(npc, nfine))
    assert (p == ptab[4, 7]).all()                                           # points 7 and 8 tie: the first


# ---- 3. end to end
INPUTS = R.end_to_end_inputs()
_HOST = {}


def host(i):
    if i not in _HOST:
        _, x, fs, plim = INPUTS[i]
        _HOST[i] = (R.model(x, fs, plim), R.model(x, fs, plim, LD))
    return _HOST[i]


@pytest.mark.parametrize("i", range(4), ids=[c[0] for c in INPUTS])
def test_end_to_end(amd, i):
    from eaqhm_amd import pitch
    name, x, fs, plim = INPUTS[i]
    m64, mld = host(i)
    plan = m64["plan"]
    pc, npc = plan["pc"], len(plan["pc"])
    dev, S = pitch.swipep_device(x, fs, plim, return_strengths=True)
    # the zero table, no unvoiced state: the raw track
    zero = dict(jump_cost=0.0, free_jump=0.0, max_jump=(npc - 1) / 96)
    assert len(pitch.viterbi_costs(npc, **zero)) == min(npc, 257)
    track, q, voiced = pitch.swipep_viterbi(x, fs, plim, return_path=True, **zero)
    raw = S.argmax(axis=0)
    edge = (raw == 0) | (raw == npc - 1)
    assert voiced.all() and track.shape == dev.shape and np.array_equal(bits(track[:, 0]), bits(dev[:, 0]))
    # (a table has at most 257 entries: on the 273 candidates of the wide inputs the path may leave the raw maximum
    # where that jumps further, which it does only from or to an instant whose raw maximum is on an edge)
    assert np.array_equal(q[~edge], raw[~edge]) and (npc > 257 or np.array_equal(q, raw))
    assert np.array_equal(bits(track[~edge, 1]), bits(dev[~edge, 1]))
    q_edge = (q == 0) | (q == npc - 1)
    assert np.array_equal(bits(track[q_edge, 1]), bits(pc[q[q_edge]]))
    bar = R.bar(np.abs(m64["s"] - mld["s"]).max())
    err = float(np.abs(track[~edge, 2] - np.asarray(mld["s"], dtype=np.float64)[~edge]).max())
    print("%s zero table: %d edge instants, strength error / bar %.3g" % (name, edge.sum(), err / bar))
    assert err <= bar and np.array_equal(bits(track[~edge, 2]), bits(dev[~edge, 2]))   # the same arithmetic: the same bits
    assert np.abs(track[q_edge, 2] - np.asarray(mld["S"], dtype=np.float64)[q[q_edge], q_edge.nonzero()[0]]).max(initial=0) \
        <= R.bar(np.abs(m64["S"] - mld["S"]).max())
    # the strength along any path against the long-double model's refinement of the device's path
    for options in (dict(), dict(unvoiced=0.2)):
        track, q, voiced = pitch.swipep_viterbi(x, fs, plim, return_path=True, **options)
        unvoiced = (0.2, 1.0) if options else None
        want = V.forward(S, pitch.viterbi_costs(npc), unvoiced, TILE)["q"]
        assert np.array_equal(q, want), options                              # the model's path on the device's own S
        assert np.array_equal(voiced, q < npc) and (voiced.all() if not options else True)
        r64 = V.refine(np.asarray(m64["S"], dtype=np.float64), q, pc, plan["ntc"], plan["nftc"], plan["ptab"], plan["nf"])
        rld = V.refine(mld["S"], q, pc, plan["ntc"], plan["nftc"], plan["ptab"], plan["nf"], LD)
        bar = max(R.bar(np.abs(r64["s"] - rld["s"]).max()), R.bar(np.abs(m64["S"] - mld["S"]).max()))
        err = float(np.abs(track[:, 2] - rld["s"]).max())
        dec = (rld["gap"] > R.GAP) & (r64["gap"] > R.GAP) & voiced
        print("%s %s: %d voiced of %d, %d steps of more than 8 candidates (raw %d), strength error / bar %.3g"
              % (name, options, voiced.sum(), len(q), V.big_steps(q, npc), V.big_steps(raw, npc), err / bar))
        record_measurement("viterbi_end_to_end_%s_%s" % (name, "uv" if options else "default"), voiced=int(voiced.sum()),
                           big_steps=V.big_steps(q, npc), big_steps_raw=V.big_steps(raw, npc), s_err_over_bar=err / bar)
        assert err <= bar
        assert np.array_equal(bits(track[dec, 1]), bits(rld["p"][dec]))
        assert np.array_equal(bits(track[:, 1]), bits(V.fill_unvoiced(track[:, 1], voiced, pc[0]))) and not track[~voiced, 2].any()
        again = pitch.swipep_viterbi(x, fs, plim, **options)
        assert np.array_equal(bits(again), bits(track))


def test_viterbi_track_on_a_host_matrix(amd):
    from eaqhm_amd import pitch
    name, S, cost, unvoiced = [c for c in CASES if c[1].shape == (273, 3 * TILE + 5) and c[3] is not None][0]
    m = V.forward(S, cost, unvoiced, TILE)
    q, last = pitch.viterbi_track(S, cost, unvoiced=unvoiced[0], voicing_cost=unvoiced[1])
    assert q.dtype == np.int32 and np.array_equal(q, m["q"]) and np.array_equal(bits(last), bits(m["last"]))
    q, last = pitch.viterbi_track(S, cost)
    assert np.array_equal(q, V.forward(S, cost, None, TILE)["q"]) and last[-1] == -np.inf


def test_analysis_from_the_viterbi_track(amd):
    from eaqhm_amd import pitch
    wav = os.path.join(GOLDEN, "SA19.WAV")
    track = pitch.analysis_pitch_track_viterbi(wav, "other")
    assert track.ndim == 2 and track.shape[1] == 3 and np.isfinite(track).all() and (track[:, 1] >= 70).all()
    srer = amd.eaQHMAnalysisAndSynthesis(wav, "other", pitch_track=track, maxAdpt=1, printPrompts=False,
                                         loadingScreen=False)[1]
    assert len(srer) >= 2 and np.isfinite(np.asarray(srer, dtype=np.float64)).all()


# ---- 4. bad arguments
def test_entry_points_refuse_bad_arguments(amd):
    """EAQHM_EINVAL (-1), nothing launched, the outputs untouched."""
    torch, c, d = ctx()
    lib, h = c.lib, c.h
    z = lambda n, dt=torch.float64: torch.zeros(n, dtype=dt, device=d)  # noqa: E731
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    outd = torch.full((64,), 7.0, dtype=torch.float64, device=d)
    outs = torch.full((256,), 7, dtype=torch.int16, device=d)
    outq = torch.full((16,), 7, dtype=torch.int32, device=d)
    S, cost, tab, nf = z(40), z(3), z(64), z(4, torch.int32)

    def fwd(S=S, npc=4, T=10, cost=cost, W=2, on=1, uv=0.2, vc=1.0, bp=outs, tm=outs[128:], last=outd):
        return lib.eaqhm_viterbi_forward(h, P(S), npc, T, P(cost), W, on, uv, vc, P(bp), P(tm), P(last))
    for bad in (dict(S=None), dict(cost=None), dict(bp=None), dict(tm=None), dict(last=None), dict(npc=2), dict(npc=1025),
                dict(T=0), dict(T=2 ** 31), dict(W=-1), dict(W=4), dict(npc=300, W=257), dict(uv=float("nan")),
                dict(vc=-1.0), dict(vc=float("inf"))):
        assert fwd(**bad) == -1, bad

    def back(bp=outs, tm=outs[128:], last=outd, npc=4, T=10, q=outq):
        return lib.eaqhm_viterbi_backtrack(h, P(bp), P(tm), P(last), npc, T, P(q))
    for bad in (dict(bp=None), dict(tm=None), dict(last=None), dict(q=None), dict(npc=2), dict(npc=1025), dict(T=0)):
        assert back(**bad) == -1, bad

    def ref(S=S, q=outq, npc=4, T=10, pc=tab, ntc=tab, nftc=tab, ptab=tab, nf=nf, nfmax=16, p=outd, s=outd[32:]):
        return lib.eaqhm_viterbi_refine(h, P(S), P(q), npc, T, P(pc), P(ntc), P(nftc), P(ptab), P(nf), nfmax, P(p), P(s))
    for bad in (dict(S=None), dict(q=None), dict(pc=None), dict(ntc=None), dict(nftc=None), dict(ptab=None), dict(nf=None),
                dict(p=None), dict(s=None), dict(npc=2), dict(npc=1025), dict(T=0), dict(nfmax=0), dict(nfmax=65)):
        assert ref(**bad) == -1, bad
    c.sync()
    assert torch.all(outd == 7.0).item() and torch.all(outs == 7).item() and torch.all(outq == 7).item()
    bp, tm, last, q = z(50, torch.int16), z(10, torch.int16), z(5), z(10, torch.int32)
    assert fwd(bp=bp, tm=tm, last=last) == 0 and fwd(bp=bp, tm=tm, last=last, on=0, uv=float("nan")) == 0
    assert back(bp=bp, tm=tm, last=last, q=q) == 0 and ref(q=q, p=z(10), s=z(10)) == 0   # good arguments run
    c.sync()
