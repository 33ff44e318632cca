"""The host side of the continuous pitch track (eaqhm_amd.pitch: viterbi_costs, viterbi_track, swipep_viterbi) and its
model (tests/viterbi_ref.py), without a GPU: the model finds what an enumeration of all paths finds, a zero cost table
gives back the raw maximum, on SA19 the path does what DESIGN.md §13.1 says it is for, and the argument checks, the
binding, the header and the CLI flags are as documented."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import swipe_ref as R  # noqa: E402
import viterbi_ref as V  # noqa: E402

PKG = os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd")
INPUTS = R.end_to_end_inputs()
_S = {}


def strengths(key):
    """The float64 model's S of an end-to-end input (0 .. 3), or of the whole of SA19 at [70, 500] ("wide"); once."""
    if key not in _S:
        _, x, fs, plim = INPUTS[key] if key != "wide" else (None, INPUTS[0][1], INPUTS[0][2], (70, 500))
        m = R.model(x, fs, plim)
        _S[key] = (np.asarray(m["S"], dtype=np.float64), m)
    return _S[key]


# ---- 1. the model against all paths
def grid(rng, npc, T, levels):
    return rng.integers(0, levels, (npc, T)) / 8.0                          # sums of these are exact


BRUTE = [(npc, T, W, uv) for npc in (3, 4) for T in (1, 2, 3, 5) for W in range(npc)
         for uv in (None, (0.25, 0.5), (0.5, 0.0))]


@pytest.mark.parametrize("npc,T,W,uv", BRUTE, ids=["npc%d-T%d-W%d-%s" % (a, b, c, "off" if d is None else "uv%g-%g" % d)
                                                    for a, b, c, d in BRUTE])
def test_model_finds_the_best_path(npc, T, W, uv):
    rng = np.random.default_rng(100 * npc + 10 * T + W)
    for levels, cost in ((64, np.arange(W + 1) / 4.0), (3, np.arange(W + 1) / 8.0), (2, np.zeros(W + 1))):
        S = grid(rng, npc, T, levels)
        m = V.forward(S, cost, uv, tile=2)
        best, paths = V.brute_force(S, cost, uv)
        assert tuple(m["q"]) in paths, (S, cost)                             # ties: one of the best, by the rules below
        assert V.score(m["q"], S, cost, uv) == best == m["last"].max()
        if len(paths) == 1:
            assert tuple(m["q"]) == paths[0]
        assert np.array_equal(V.path_from_tilemap(m, T, tile=2), m["q"])


def test_model_ties_by_rule():
    cost = np.zeros(3)
    S = np.array([[1.0, 0.0], [0.0, 0.0], [1.0, 0.0], [0.0, 0.0], [1.0, 0.0]])
    m = V.forward(S, cost)
    assert list(m["bp"][1, :5]) == [0, 0, 2, 2, 4]                           # the smaller |c - c'|, then the lower c'
    assert list(m["q"]) == [0, 0]                                            # the first maximum at the end
    m = V.forward(np.zeros((4, 3)), np.zeros(2), (0.0, 0.0))
    assert list(m["bp"][1]) == [0, 1, 2, 3, 4] and list(m["q"]) == [0, 0, 0]  # the unvoiced state only if strictly better
    m = V.forward(np.zeros((4, 3)), np.zeros(2), (0.125, 0.0))
    assert list(m["q"]) == [4, 4, 4] and m["last"][4] == 0.375
    m = V.forward(np.array([[0.0, 1.0], [0.0, 1.0], [0.5, 0.0]]), np.zeros(1), (0.0, 0.25))
    assert m["bp"][1, 3] == 2 and m["last"][3] == 0.25                       # entered from the first maximum of D[., 0]


# ---- 2. a zero table gives the raw track back
@pytest.mark.parametrize("i", range(4), ids=[c[0] for c in INPUTS])
def test_zero_table_is_the_raw_maximum(i):
    S, m = strengths(i)
    q = V.forward(S, np.zeros(S.shape[0]))["q"]
    print("%s: %d differences, least leading gap %.2e" % (INPUTS[i][0], (q != m["i"]).sum(), m["gap1"].min()))
    assert np.array_equal(q, m["i"]) and np.array_equal(q, V.raw_path(S))


# ---- 3. what the path is for, on SA19 at [70, 500] with the defaults
def test_sa19_wide_range():
    from eaqhm_amd import pitch
    S, m = strengths("wide")
    npc = S.shape[0]
    pc = m["plan"]["pc"]
    cost = pitch.viterbi_costs(npc)
    W = len(cost) - 1
    raw = V.raw_path(S)
    q = V.forward(S, cost)["q"]
    assert W == 48 and np.abs(np.diff(q)).max() <= W
    steps_raw, steps = V.big_steps(raw, npc), V.big_steps(q, npc)
    print("steps of more than 8 candidates: raw %d, path %d" % (steps_raw, steps))
    assert 10 * steps <= steps_raw
    Sn, mn = strengths(0)                                                    # the [160, 300] track
    pn = mn["plan"]["pc"][V.raw_path(Sn)]
    sel = (Sn.max(axis=0) > 0.3) & (pn >= 165) & (pn <= 290)
    agree = lambda path: int((np.abs(np.log2(pc[path][sel] / pn[sel])) <= 0.03).sum())  # noqa: E731
    print("agreement with the [160, 300] track at %d instants: raw %d, path %d" % (sel.sum(), agree(raw), agree(q)))
    assert sel.sum() > 1000 and agree(q) >= agree(raw)
    qv = V.forward(S, cost, (0.2, 1.0))["q"]
    changes, changes_raw = V.voicing_changes(qv < npc), V.voicing_changes(S.max(axis=0) > 0.2)
    print("voicing changes: threshold %d, path %d" % (changes_raw, changes))
    assert changes < changes_raw and 0 < (qv < npc).sum() < len(qv)


# ---- 4. the cost table, the checks, the fill rule
def test_viterbi_costs():
    from eaqhm_amd import pitch
    c = pitch.viterbi_costs(273)
    assert c.dtype == np.float64 and len(c) == 49 and not c[:3].any() and c[3] == 4.0 / 96 and c[48] == 4.0 * 46 / 96
    assert np.array_equal(c, 4.0 * np.maximum(0, np.arange(49) - 2) / 96)
    assert len(pitch.viterbi_costs(20)) == 20 and len(pitch.viterbi_costs(1024, max_jump=5.0)) == 257
    assert np.array_equal(pitch.viterbi_costs(87, 0.0), np.zeros(49))
    assert np.array_equal(pitch.viterbi_costs(87, 2.0, 0.0, 0.0), np.zeros(1))
    assert np.array_equal(pitch.viterbi_costs(5, 96.0, 0.0, 1.0), np.arange(5.0))
    for bad in (dict(npc=2), dict(npc=1025), dict(npc=3.5), dict(npc=True), dict(jump_cost=-1), dict(jump_cost=np.nan),
                dict(jump_cost="x"), dict(free_jump=-0.1), dict(free_jump=0.6), dict(max_jump=np.inf), dict(max_jump=-1),
                dict(free_jump=None)):
        args = dict(npc=87)
        args.update(bad)
        with pytest.raises(ValueError):
            pitch.viterbi_costs(**args)
    with pytest.raises(ValueError, match="1024"):
        pitch.viterbi_costs(1025)


TRACK_BAD = (
    (dict(S=np.zeros(5)), "2-D"), (dict(S=np.zeros((2, 5))), "1024"), (dict(S=np.zeros((1025, 2))), "1024"),
    (dict(S=np.zeros((5, 0))), "instants"), (dict(S=np.full((5, 3), np.nan)), "finite"),
    (dict(S=np.array([[0.0, np.inf]] * 3)), "finite"), (dict(S=np.zeros((3, 3), dtype=complex)), "real"),
    (dict(cost=np.zeros(6)), "cost"), (dict(cost=np.zeros(0)), "cost"), (dict(cost=np.zeros((2, 2))), "cost"),
    (dict(cost=np.array([0.0, -1.0])), "cost"), (dict(cost=np.array([0.0, np.nan])), "cost"),
    (dict(S=np.zeros((300, 2)), cost=np.zeros(258)), "cost"), (dict(unvoiced=np.nan), "unvoiced"),
    (dict(unvoiced="x"), "unvoiced"), (dict(unvoiced=0.2, voicing_cost=-1.0), "voicing_cost"),
    (dict(unvoiced=0.2, voicing_cost=np.inf), "voicing_cost"), (dict(device_index=-1), "device_index"),
    (dict(device_index=0.5), "device_index"),
)


@pytest.mark.parametrize("change,match", TRACK_BAD, ids=[str(n) for n in range(len(TRACK_BAD))])
def test_viterbi_track_refuses(change, match, monkeypatch):
    from eaqhm_amd import pitch, records
    monkeypatch.setattr(records, "_device", lambda *a: pytest.fail("device work before the checks"))
    args = dict(S=np.zeros((5, 4)), cost=np.zeros(3))
    args.update(change)
    S, cost = args.pop("S"), args.pop("cost")
    with pytest.raises(ValueError, match=match):
        pitch.viterbi_track(S, cost, **args)


SWIPE_BAD = (
    (dict(x=np.array([0.0, np.nan])), "finite"), (dict(plim=(300, 160)), "plim"), (dict(jump_cost=-1.0), "jump_cost"),
    (dict(free_jump=1.0), "free_jump"), (dict(max_jump=np.nan), "max_jump"), (dict(unvoiced=np.inf), "unvoiced"),
    (dict(unvoiced=0.2, voicing_cost=-0.5), "voicing_cost"), (dict(device_index=-2), "device_index"),
)


@pytest.mark.parametrize("change,match", SWIPE_BAD, ids=[str(n) for n in range(len(SWIPE_BAD))])
def test_swipep_viterbi_refuses(change, match, monkeypatch):
    from eaqhm_amd import pitch, records
    monkeypatch.setattr(records, "_device", lambda *a: pytest.fail("device work before the checks"))
    monkeypatch.setattr(pitch, "_device_plan", lambda *a: pytest.fail("device work before the checks"))
    args = dict(x=np.zeros(800), fs=16000, plim=(160, 300))
    args.update(change)
    x, fs, plim = args.pop("x"), args.pop("fs"), args.pop("plim")
    with pytest.raises(ValueError, match=match):
        pitch.swipep_viterbi(x, fs, plim, **args)


def test_too_many_candidates_names_the_limit(monkeypatch):
    """SWIPE's own limits (8 window sizes, 8192 samples) keep its grids below 1024 candidates, so the guard of
    swipep_viterbi is met here with the limit lowered; viterbi_track meets the real one above."""
    from eaqhm_amd import pitch, records
    monkeypatch.setattr(records, "_device", lambda *a: pytest.fail("device work before the checks"))
    monkeypatch.setattr(pitch, "VITERBI_NPC_MAX", 50)
    with pytest.raises(ValueError, match="88 pitch candidates, the limit of the decode is 50"):
        pitch.swipep_viterbi(np.zeros(800), 16000, (160, 300))
    with pytest.raises(ValueError):
        pitch.analysis_pitch_track_viterbi("x.wav", "other", return_path=True)


def test_fill_unvoiced():
    from eaqhm_amd import pitch
    p = np.array([0.0, 0.0, 110.0, 0.0, 0.0, 220.0, 230.0, 0.0])
    v = p > 0
    want = np.array([110.0, 110.0, 110.0, 110.0, 110.0, 220.0, 230.0, 230.0])
    assert np.array_equal(pitch.fill_unvoiced(p, v, 70.0), want) and np.array_equal(V.fill_unvoiced(p, v, 70.0), want)
    assert np.array_equal(pitch.fill_unvoiced(p, np.zeros(8, dtype=bool), 70.0), np.full(8, 70.0))
    assert np.array_equal(pitch.fill_unvoiced(p, np.ones(8, dtype=bool), 70.0), p)
    rng = np.random.default_rng(0)
    for _ in range(20):
        p = rng.uniform(70, 500, 30)
        v = rng.random(30) < 0.4
        assert np.array_equal(pitch.fill_unvoiced(p, v, 70.0), V.fill_unvoiced(p, v, 70.0))


# ---- 5. symbols, header, Makefile, the unchanged surface
def test_symbols_header_and_makefile():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import hip, pitch
    counts = dict(eaqhm_viterbi_forward=12, eaqhm_viterbi_backtrack=7, eaqhm_viterbi_refine=13)
    assert hip.ABI_VERSION == 6
    bound = {name: len(args) for name, _, args in hip.SYMBOLS_VITERBI}
    others = (hip.SYMBOLS + hip.SYMBOLS_MLPG + hip.SYMBOLS_GV + hip.SYMBOLS_CEPWARP + hip.SYMBOLS_KMEANS
              + hip.SYMBOLS_MLPG_EM + hip.SYMBOLS_NN + hip.SYMBOLS_SWIPE)
    assert not set(bound) & {name for name, _, _ in others}
    header = open(os.path.join(ROOT, "include", "eaqhm_viterbi.h")).read()
    assert '#include "eaqhm_viterbi.h"' in open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t)\s+(eaqhm_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(bound) == set(counts)
    for name, n in counts.items():
        assert bound[name] == n, name
        decl = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, header, re.M)
        assert decl is not None and len(decl.group(1).split(",")) == n, name
    for name in ("viterbi_forward", "viterbi_backtrack", "viterbi_refine"):
        assert callable(getattr(hip.Context, name))
    for const, macro in (("VITERBI_TILE", "EAQHM_VITERBI_TILE"), ("VITERBI_NPC_MAX", "EAQHM_VITERBI_NPC"),
                         ("VITERBI_JUMP_MAX", "EAQHM_VITERBI_JUMP")):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, header).group(1)) == getattr(pitch, const)
    lib = hip.load_library()                                                 # a null context: EAQHM_EINVAL
    assert lib.eaqhm_viterbi_forward(None, None, 3, 1, None, 0, 0, 0.0, 0.0, None, None, None) == -1
    assert lib.eaqhm_viterbi_backtrack(None, None, None, None, 3, 1, None) == -1
    assert lib.eaqhm_viterbi_refine(None, None, None, 3, 1, None, None, None, None, None, 1, None, None) == -1
    makefile = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\beaqhm_viterbi\.hip\b", makefile, re.M)
    assert re.search(r"^HDR\s*:=.*include/eaqhm_viterbi\.h\b", makefile, re.M)
    unit = open(os.path.join(PKG, "csrc", "eaqhm_viterbi.hip")).read()
    assert "#pragma clang fp contract(off)" in unit and "atomic" not in unit.replace("No atomics", "")


def test_surface():
    import eaqhm_amd
    from eaqhm_amd import pitch
    for name in ("swipep_viterbi", "viterbi_costs", "viterbi_track", "analysis_pitch_track_viterbi"):
        assert callable(getattr(pitch, name)) and not hasattr(eaqhm_amd, name)
    assert "§13.1" in pitch.__doc__
    assert str(inspect.signature(pitch.swipep_device)) == "(x, fs, plim, *, device_index=0, return_strengths=False)"
    assert str(inspect.signature(pitch.analysis_pitch_track)) == "(speechFile, gender, fc=0, *, device_index=0)"
    sig = inspect.signature(pitch.swipep_viterbi)
    assert list(sig.parameters) == ["x", "fs", "plim", "jump_cost", "free_jump", "max_jump", "unvoiced", "voicing_cost",
                                    "device_index", "return_path"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == [4.0, 1 / 48, 0.5, None, 1.0, 0, False]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[3:])
    assert str(inspect.signature(pitch.viterbi_track)) == "(S, cost, *, unvoiced=None, voicing_cost=1.0, device_index=0)"
    assert str(inspect.signature(pitch.analysis_pitch_track_viterbi)) == \
        "(speechFile, gender, fc=0, *, device_index=0, **options)"


# ---- 6. the CLI
def test_cli_flags(monkeypatch):
    from eaqhm_amd import cli, pitch
    a = cli.parser().parse_args(["x.wav"])
    assert a.pitch_viterbi is False and a.pitch_jump_cost is None and a.pitch_unvoiced is None
    a = cli.parser().parse_args(["x.wav", "--pitch-viterbi", "--pitch-jump-cost", "2.5", "--pitch-unvoiced", "0.2"])
    assert a.pitch_viterbi is True and cli.viterbi_options(a) == dict(jump_cost=2.5, unvoiced=0.2)
    assert cli.viterbi_options(cli.parser().parse_args(["x.wav", "--pitch-viterbi"])) == {}
    for flag in ("--pitch-viterbi", "--pitch-jump-cost", "--pitch-unvoiced"):
        assert flag in cli.__doc__
    seen = []
    monkeypatch.setattr(cli, "eaQHMAnalysisAndSynthesis", lambda path, gender, **o: seen.append((path, o)) or "result")
    monkeypatch.setattr(pitch, "analysis_pitch_track", lambda *a, **k: pytest.fail("the per-instant tracker ran"))
    monkeypatch.setattr(pitch, "analysis_pitch_track_viterbi",
                        lambda path, gender, fc=0, **o: ("viterbi track of", path, gender, fc, o))
    assert cli.analyse("a.wav", "male", dict(step=15, fc=3)) == "result"      # without the flag: the call as it was
    assert cli.analyse("b.wav", "male", dict(step=15, fc=3, pitch_viterbi={})) == "result"
    assert cli.analyse("c.wav", "other", dict(step=15, pitch_device=True, pitch_viterbi=dict(unvoiced=0.2))) == "result"
    assert seen == [("a.wav", dict(step=15, fc=3)),
                    ("b.wav", dict(step=15, fc=3, pitch_track=("viterbi track of", "b.wav", "male", 3, {}))),
                    ("c.wav", dict(step=15, pitch_track=("viterbi track of", "c.wav", "other", 0, dict(unvoiced=0.2))))]
    for argv in (["x.wav", "--pitch-jump-cost", "2"], ["x.wav", "--pitch-unvoiced", "0.2"],
                 ["x.wav", "--pitch-viterbi", "--pitch-jump-cost", "-1"],
                 ["x.wav", "--pitch-viterbi", "--pitch-unvoiced", "nan"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
    assert seen[3:] == []                                                    # refused before any analysis
