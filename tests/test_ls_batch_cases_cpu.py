"""The cases of tests/ls_batch_ref.py and their NumPy reference, checked without a GPU.

Three things keep the GPU test (tests/test_gpu_ls_batch_direct.py) honest:
  coverage      the tags of every set hold every shape and edge the set promises, so an edit of a builder cannot lose one
  conditioning  every frame's normal equations solved three ways (inv(), Cholesky, QR least squares on the weighted
                basis) agree to 1/10 of the GPU bars: 1e-10 of the frame's largest amplitude, 1e-9 of its largest slope;
                and no reference cell lies within 1e-6 (relative) of an acceptance threshold, so the acceptance masks of
                two correct implementations agree
  model         OracleBackend.ls_batch equals oracle.Analysis.ls_stage (record rows) and oracle.eaqhm_ls (raw solutions)
                on the same dense arrays"""
import functools

import numpy as np
import pytest

import eaqhm_oracle as O
import ls_batch_ref as R

BAR_AMP, BAR_SLOPE = 1e-10, 1e-9          # 1/10 of the GPU bars (test_gpu_parity.py: 1e-9 / 1e-8)


@functools.lru_cache(maxsize=None)
def built(name):
    case = R.BUILDERS[name]()
    with R.one_thread():
        return case, R.run(case)


# ------------------------------------------------------------------------------------------------ coverage
def test_set_S_covers_every_size_and_last_chunk_shape():
    case = built("S")[0]
    tags = case["tags"]
    assert case["Kmax"] == 56 and case["mode"] == 1
    assert sorted({t["n"] for t in tags}) == R.S_SIZES
    assert sorted({t["nt"] for t in tags if t["n"] <= 51}) == list(range(1, 14))
    assert {t["nt"] for t in tags if t["n"] > 51} == {14, 15}                 # the large-frame class
    for cls in list(range(1, 14)) + ["big"]:
        shapes = {(t["wl"] + 1) % 16 for t in tags if (t["nt"] if t["nt"] <= 13 else "big") == cls}
        assert shapes == set(range(16)), cls
    for n in (1, 8, 30, 51):
        assert {400, 511} <= {t["wl"] for t in tags if t["n"] == n}
    assert max(t["wl"] for t in tags) == 511                                  # N = 1023, the tile kernel's limit
    assert np.mean([t["holes"] for t in tags]) >= 1 / 3
    for f, t in enumerate(tags):                                              # `holes` says what frame_prep finds
        cols = built("S")[1]["cols"][f, :t["n"]]
        assert t["holes"] == (not np.array_equal(cols, np.arange(t["n"])))
        assert t["gap"] == "none" and not t["seeded"]
    fm, c, wl = case["fm"], case["frame_c"], case["frame_wl"]
    for f, t in enumerate(tags):                                              # no zero inside any window, nor before it
        act = fm[:, c[f]] != 0
        assert (fm[act, c[f] - wl[f] - 1:c[f] + wl[f] + 1] != 0).all()


def _gap_words(case, ref, f):
    """(zero mask [n][N] of the active slots over the window, zero on the sample before the window [n])."""
    c, wl = int(case["frame_c"][f]), int(case["frame_wl"][f])
    act = ref["cols"][f, :ref["ncol"][f]]
    return case["fm"][act, c - wl:c + wl + 1] == 0, case["fm"][act, c - wl - 1] == 0


def _runs(z):
    """[lo, hi) runs of True in a boolean vector."""
    d = np.diff(np.concatenate(([0], z.astype(int), [0])))
    return list(zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)))


def test_set_G_covers_every_gap_kind_at_every_size():
    case, ref = built("G")
    tags = case["tags"]
    assert {(t["n"], t["gap"]) for t in tags} == {(n, k) for n in R.G_SIZES for k in R.GAP_KINDS}
    # one size per class of frame_class (nt <= 8, 9, 10, 11, 12, 13) plus the large class
    assert [R.tile_rows(n) for n in R.G_SIZES] == [1, 4, 8, 10, 11, 12, 13, 14]
    for f, t in enumerate(tags):
        z, before = _gap_words(case, ref, f)
        wl = t["wl"]
        N = 2 * wl + 1
        assert not z[:, wl].any()                                             # the centre sample stays nonzero
        gappy = np.flatnonzero(z.any(axis=1))
        kind = t["gap"]
        if kind == "all_slots":
            assert len(gappy) == t["n"]
            continue
        if kind == "outside":                                                 # only the sample before the window
            assert len(gappy) == 0 and before.sum() == 1
            continue
        assert len(gappy) == 1 and not before.any()
        runs = _runs(z[gappy[0]])
        assert len(runs) == (2 if kind == "two_gaps" else 1)
        lo, hi = runs[0]
        if kind == "lead":
            assert lo == 0 and 1 < hi < wl
        elif kind == "trail":
            assert hi == N and wl < lo < N - 1
        elif kind == "one":
            assert hi - lo == 1 and 0 < lo < N - 1
        elif kind == "word":
            assert lo % 64 == 0 and hi - lo == 64 and lo > 0
        elif kind == "two_words":
            assert lo % 64 == 0 and hi - lo == 128 and lo > 0
        elif kind == "from_bit0":
            assert lo % 64 == 0 and (hi - lo) < 64 and hi % 64 != 0 and lo > 0
        elif kind == "to_bit63":
            assert hi % 64 == 0 and (hi - lo) < 64 and lo % 64 != 0 and hi < N
        elif kind == "first":
            assert (lo, hi) == (0, 1)
        elif kind == "last":
            assert (lo, hi) == (N - 1, N)
        elif kind == "two_gaps":
            assert lo > 0 and runs[1][1] < N and runs[1][0] > wl > hi          # one on each side of the centre


def test_set_P_places_frames_on_every_boundary():
    case, ref = built("P")
    t0, tl = case["track_t0"], case["track_len"]
    c, wl, tags = case["frame_c"].astype(int), case["frame_wl"].astype(int), case["tags"]
    place = [t["place"] for t in tags]
    assert t0 % 1024 != 0 and t0 + tl < case["L"] - 1000 and case["dropped"] == 1
    assert any(c[f] - wl[f] - 1 == t0 for f in range(len(c)) if place[f] == "first")
    assert any(c[f] + wl[f] == t0 + tl - 1 for f in range(len(c)) if place[f] == "last")
    k = case["boundary_slot"]
    assert np.array_equal(np.flatnonzero(case["fm_full"][k, 1500:3000] == 0) + 1500, [2047, 2048])
    ka, kb = case["side_slots"]                                               # and one slot for each side alone
    assert list(np.flatnonzero(case["fm_full"][ka, 1500:3000] == 0) + 1500) == [2047]
    assert list(np.flatnonzero(case["fm_full"][kb, 1500:3000] == 0) + 1500) == [2048]
    strad = [f for f in range(len(c)) if place[f] == "straddle"]
    assert all(c[f] - wl[f] <= 2047 and c[f] + wl[f] >= 2048 for f in strad)
    assert {int(c[f]) for f in strad} >= {2047, 2048}                         # the slot leaves the frames centred on its zeros
    assert sum(k in ref["cols"][f, :ref["ncol"][f]] for f in strad) == len(strad) - 2
    assert all(sum(q in ref["cols"][f, :ref["ncol"][f]] for f in strad) == len(strad) - 1 for q in (ka, kb))
    k = case["chunk_slot"]
    assert (case["fm_full"][k, 3072:4096] == 0).all() and case["fm_full"][k, 3071] != 0 and case["fm_full"][k, 4096] != 0
    f = place.index("chunk_after")
    assert c[f] - wl[f] - 1 == 4095 and k in ref["cols"][f, :ref["ncol"][f]]  # reads the count 1024 (and subtracts it)
    f = place.index("chunk_lead")
    assert 3072 <= c[f] - wl[f] - 1 < 4095 and c[f] + wl[f] >= 4096 and k in ref["cols"][f, :ref["ncol"][f]]
    f = place.index("chunk_before")
    assert c[f] + wl[f] == 3071
    f = place.index("dropped")
    assert f == len(c) - 1 and c[f] - wl[f] == t0 - 1
    inside = (c - wl - 1 >= t0) & (c + wl < t0 + tl)
    assert inside[:-1].all() and not inside[-1]
    assert np.all(np.diff(c[:-1]) > 0)


def test_set_P0_starts_on_sample_zero():
    case = built("P0")[0]
    c, wl = case["frame_c"].astype(int), case["frame_wl"].astype(int)
    assert case["track_t0"] == 0 and case["track_len"] == case["L"] and case["dropped"] == 0
    assert (c - wl == 0).any() and (c - wl - 1 == 0).any()
    k = case["boundary_slot"]
    assert np.array_equal(np.flatnonzero(case["fm"][k, :2000] == 0), [1023, 1024])
    ka, kb = case["side_slots"]
    assert list(np.flatnonzero(case["fm"][ka, :2000] == 0)) == [1023] and list(np.flatnonzero(case["fm"][kb, :2000] == 0)) == [1024]
    strad = [f for f, t in enumerate(case["tags"]) if t["place"] == "straddle"]
    assert len(strad) == 4 and all(c[f] - wl[f] <= 1023 and c[f] + wl[f] >= 1024 for f in strad)
    assert case["f0_stale"] < case["f0min"]                                   # functions.py:321: no frequency correction


def test_set_E_seeds_and_shows_them_to_the_right_neighbours():
    case, ref = built("E")
    c, wl, tags = case["frame_c"].astype(int), case["frame_wl"].astype(int), case["tags"]
    assert np.all(np.diff(c) > 0)                                             # the sequential loop's order
    seeds = ref["seeded"]
    assert list(seeds) == [int(c[f]) for f, t in enumerate(tags) if t["seeded"]] and len(seeds) == 6
    assert set(case["empty"]) < set(seeds)
    seen = set()
    for f, t in enumerate(tags):
        inwin = seeds[(seeds >= c[f] - wl[f]) & (seeds <= c[f] + wl[f])]
        slot0 = 0 in ref["cols"][f, :ref["ncol"][f]]
        if t["seeded"]:
            assert ref["ncol"][f] == 1 and slot0
        if t["role"] == "seed_before_centre":
            assert (inwin < c[f]).any()
            seen.add(("before", slot0))
        if t["role"] == "seed_after_centre":
            assert (inwin > c[f]).all() and len(inwin)
            seen.add(("after", slot0))
        if t["role"] == "clear":
            assert len(inwin) == 0
        if t["seeded"] and len(inwin) > 1:
            seen.add("two seeds in one seeded window")
        if t["seeded"] and not case["fm"][0, c[f] - wl[f]:c[f] + wl[f] + 1].any():
            seen.add("slot 0 empty but for the seeds")
    # (.., True): the seeded sample lies inside a slot 0 that is otherwise active
    assert seen == {("before", True), ("before", False), ("after", True), ("after", False),
                    "two seeds in one seeded window", "slot 0 empty but for the seeds"}


@pytest.mark.parametrize("name, fs, Kmax, Ks", [("Z16", 16000, 60, R.Z16_K), ("Z48", 48000, 170, R.Z48_K)])
def test_set_Z_frame_K_list(name, fs, Kmax, Ks):
    case = built(name)[0]
    assert case["mode"] == 0 and case["fs"] == fs and case["Kmax"] == Kmax and case["a_iter"] == 0
    assert sorted(set(case["frame_K"].tolist())) == list(Ks)
    assert np.all(case["frame_K"] * case["frame_f0"] <= fs / 2 - 200)
    want = np.maximum(120, np.round(1.5 * fs / case["frame_f0"]))             # wl as in the product (functions.py:191)
    assert np.abs(case["frame_wl"] - want).max() <= 1                         # (the second frame's pitch is 0.2 % off)
    if name == "Z48":                                                         # both sides of MF_A0_M = 19 real tile rows
        rows = (2 * case["frame_K"] + 2 + 15) >> 4
        assert {int(r) for r in rows} == {13, 19, 20, 22}
    else:
        assert 2 * case["wl_max"] + 1 <= 1024


def test_set_B_is_large_frames_only():
    case, ref = built("B")
    tags = case["tags"]
    c, wl = case["frame_c"].astype(int), case["frame_wl"].astype(int)
    assert case["Kmax"] == 80 and 2 * case["wl_max"] + 1 > 1024 and case["wl_max"] == 560
    assert {t["n"] for t in tags} == set(R.B_SIZES) and min(t["nt"] for t in tags) >= 14
    two = [f for f, t in enumerate(tags) if t.get("place") == "two_boundaries" or t["gap"] == "two_boundaries_gap"]
    assert len(two) == 2
    for f in two:
        assert 2 * wl[f] + 1 >= 1025 and ((c[f] + wl[f]) >> 10) - ((c[f] - wl[f] - 1) >> 10) == 2
    gappy = [f for f in range(len(c)) if _gap_words(case, ref, f)[0].any()]
    assert gappy == [f for f, t in enumerate(tags) if t["gap"] != "none"] and len(gappy) == 2
    for f in gappy:
        assert not _gap_words(case, ref, f)[0][:, wl[f]].any()
    # the gappy window over two boundaries: slots whose only zeros lie in the first, the middle, the last of its three chunks
    f = [f for f in gappy if tags[f]["gap"] == "two_boundaries_gap"][0]
    z = _gap_words(case, ref, f)[0]
    chunk = (np.arange(c[f] - wl[f], c[f] + wl[f] + 1) >> 10) - ((c[f] - wl[f] - 1) >> 10)
    alone = {tuple(np.unique(chunk[row])) for row in z if row.any()}
    assert {(0,), (1,), (2,)} <= alone and len(alone) == 4


def test_tile_path_sets_stay_inside_it():
    """Nmax <= 64 * CI_NCH = 1024 is the one condition of ls_tile_applicable these sets can break (its LDS term allows
    Kmax <= 229: see the docstring of tests/test_gpu_ls_batch_direct.py); B breaks it on purpose."""
    for name in ("S", "G", "P", "P0", "E", "Z16"):
        case = built(name)[0]
        assert 2 * case["wl_max"] + 1 <= 1023 and case["Kmax"] <= 60, name


# ------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("name", [pytest.param("S", marks=pytest.mark.slow), "G", "P", "P0", "E", "Z16", "Z48", "B"])
def test_three_solves_agree_and_no_cell_sits_on_a_threshold(name):
    case, ref = built(name)
    worst = np.zeros(2)
    live = case["n_frames"] - case["dropped"]
    done = 0
    with R.one_thread():
        for f, Ew, ws in R.systems(case, ref):
            n = case["tags"][f]["n"]
            Kc = 2 * n + 1
            assert Ew.shape[1] == 2 * Kc
            x = R.three_solves(Ew, ws)
            assert np.array_equal(x[0][:Kc], ref["raw_amp"][f, :Kc]) and np.array_equal(x[0][Kc:], ref["raw_slope"][f, :Kc])
            assert np.isnan(ref["raw_amp"][f, Kc:]).all()
            sa, ss = np.abs(x[0][:Kc]).max(), np.abs(x[0][Kc:]).max()
            for u, v in ((0, 1), (0, 2), (1, 2)):
                ea, es = np.abs(x[u][:Kc] - x[v][:Kc]).max() / sa, np.abs(x[u][Kc:] - x[v][Kc:]).max() / ss
                assert ea <= BAR_AMP and es <= BAR_SLOPE, (name, f, case["tags"][f], u, v, ea, es)
                worst = np.maximum(worst, (ea, es))
            # the two acceptance tests (functions.py:309-315) of the positive slots
            A, B = x[0][n + 1:Kc], x[0][Kc + n + 1:]
            mag = np.abs(A)
            assert np.all(np.abs(mag / (mag.max() * 10 ** -7.5) - 1) > 1e-6)
            if case["mode"] == 1:
                eta = case["fs"] / (2 * np.pi) * (A.real * B.imag - A.imag * B.real) / mag ** 2
                assert np.all(np.abs(np.abs(eta) / (case["f0_stale"] / (case["a_iter"] + 1)) - 1) > 1e-6)
            done += 1
    assert done == live
    print("%s: three solves within %.1e (amplitudes) / %.1e (slopes) of each other" % (name, worst[0], worst[1]))


# ------------------------------------------------------------------------------------------------ model against oracle
@pytest.mark.parametrize("name", [pytest.param("S", marks=pytest.mark.slow), "G", "E"])
def test_model_equals_the_oracle(name):
    case, ref = built(name)
    K, nf = case["Kmax"], case["n_frames"]
    assert case["track_t0"] == 0 and case["track_len"] == case["L"] and case["dropped"] == 0
    an = object.__new__(O.Analysis)
    an.s, an.fs, an.Kmax, an.No_ti, an.f0min = case["s"], case["fs"], K, case["n_rows"], case["f0min"]
    an.ti = np.zeros(an.No_ti, dtype=np.int64)
    an.voiced = np.zeros(an.No_ti, dtype=bool)
    an.wls = np.zeros(an.No_ti, dtype=np.int64)
    inst = case["frame_inst"]
    assert np.all(np.diff(inst) > 0)
    an.ti[inst], an.voiced[inst], an.wls[inst] = case["frame_c"] + 1, True, case["frame_wl"]
    an.f0_stale, an.n_ls = case["f0_stale"], 0
    an.fm_current, an.am_current = case["fm"].T.copy(), case["am"].T.copy()
    with R.one_thread():
        rec = an.ls_stage(case["a_iter"])
        assert list(an.seeded) == list(ref["seeded"]) and an.n_ls == nf
        got = ref["records"]
        assert np.array_equal(got[inst, :K], rec["am"][inst]) and np.array_equal(got[inst, K:2 * K], rec["fm"][inst])
        assert np.array_equal(got[inst, 2 * K:3 * K], rec["ph"][inst]) and np.array_equal(got[inst, 3 * K], rec["a0"][inst])
        other = np.setdiff1d(np.arange(an.No_ti), inst)
        assert len(other) == 3 and np.isnan(got[other]).all()
        assert (rec["am"][inst] != 0).any(axis=1).all()
        for f, sig, AM, FM in R.frame_inputs(case, ref):
            amp, slo = O.eaqhm_ls(sig, AM, FM, np.hamming(len(sig)), case["fs"])
            Kc = len(amp)
            assert np.array_equal(ref["raw_amp"][f, :Kc], amp) and np.array_equal(ref["raw_slope"][f, :Kc], slo)
