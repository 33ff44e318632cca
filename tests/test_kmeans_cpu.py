"""CPU tests of the k-means codebook: the NumPy model's own properties (tests/kmeans_ref.py), the
conditions on every input set of tests/test_gpu_kmeans.py, the host side of eaqhm_amd.convert (every argument check, the
loop driven through a NumPy stand-in for the two kernels, init="kmeans"), the new symbols and the CLI flag.  No GPU.

The quality case (kmeans_ref.polytope(3, seed=3): six blobs of 100 rows at +-3 e_j, sigma 0.5, shuffled; gmm_ref.fit, 20
rounds, tol = 0): the axis start ends at a mean log-likelihood of -4.354867, the k-means start at -3.895601.  With
polytope(4, seed=4) and 8 components: -5.224871 against -4.854331."""
import os
import re

import numpy as np
import pytest

import gmm_ref as G
import kmeans_ref as K
from conftest import ROOT

LD = np.longdouble


@pytest.fixture()
def no_device(monkeypatch):
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import functions

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(functions, "_ctx", boom)


_LOOP = {}


def loop(name):
    if name not in _LOOP:
        Z, k, split, scale = K.loop_case(name)
        R, zbar, sd = K.rows(Z, split, scale)
        _LOOP[name] = (Z, k, split, scale, R, zbar, sd, K.kmeans(R, k), K.kmeans(R, k, dtype=LD))
    return _LOOP[name]


# ---- the model against itself
@pytest.mark.parametrize("name", ["polytope3", "corners5"])
def test_model_sse_never_rises_at_fixed_k(name):
    for f in loop(name)[7:]:
        hist = f["sse_history"]
        assert len(hist) == f["rounds"] >= 3
        for (k0, s0), (k1, s1) in zip(hist, hist[1:]):
            if k0 == k1:
                assert s1 <= s0 * (1 + 1e-14), (k0, s0, s1)
        assert float(f["sse"].sum()) <= float(hist[-1][1]) * (1 + 1e-14)
        assert hist[0][0] == 2 and hist[-1][0] == loop(name)[1]


@pytest.mark.parametrize("name", ["polytope3", "corners5"])
def test_model_precisions_agree_where_decided(name):
    _, k, _, _, R, _, _, f, g = loop(name)
    assert len(f["assigns"]) == len(g["assigns"])
    for (C, lab), (Cl, labl) in zip(f["assigns"], g["assigns"]):
        ok = K.decided(R, C) & K.decided(R, Cl)
        assert np.array_equal(lab[ok], labl[ok]) and ok.all()
    assert np.array_equal(f["labels"], g["labels"]) and np.array_equal(f["counts"], np.bincount(f["labels"], minlength=k))
    assert f["counts"].min() > 0


@pytest.mark.parametrize("i", range(len(K.ASSIGN_SHAPES)))
def test_assign_inputs_are_decided(i):
    """A condition on the inputs of the GPU test: the undecided share is at most 1 %; with these seeds it is 0."""
    Z, C = K.assign_case(i)
    N, D, Kc, ldz = K.ASSIGN_SHAPES[i]
    assert Z.shape == (N, ldz or D) and C.shape == (Kc, D) and np.all(np.isnan(Z[:, D:])) and np.all(np.isfinite(Z[:, :D]))
    ok = K.decided(Z[:, :D], C)
    assert (~ok).sum() <= 0.01 * N and ok.all()
    assert np.array_equal(K.assign(Z[:, :D], C)[ok], K.assign(Z[:, :D], C, LD)[ok])


def test_assign_shapes_cover_the_edges():
    Ns, Ds, Ks = ({s[i] for s in K.ASSIGN_SHAPES} for i in range(3))
    assert Ns == {1, 63, 64, 65, 129} and Ds == {1, 3, 4, 5, 16, 17, 64, 127, 128} and Ks == {1, 2, 15, 16, 17, 63, 64}
    assert any(s[3] for s in K.ASSIGN_SHAPES)


def test_ties_give_the_lowest_index():
    Z, C = K.tie_case()
    assert np.array_equal(C[3], C[20]) and np.array_equal(C[5], C[37])
    for dtype in (np.float64, LD):
        lab = K.assign(Z, C, dtype)
        assert lab[0] == 38 and lab[1 + 3] == 3 and lab[1 + 20] == 3 and lab[1 + 5] == 5 and lab[1 + 37] == 5
    s = K.scores(Z, C)
    assert s[0, 38] == s[0, 39] == s[0].min()                         # the row half way between two centres
    assert np.array_equal(s, np.round(s)) and np.array_equal(s.astype(LD), K.scores(Z, C, LD))   # integers: exact
    assert not K.decided(Z, C)[0]                                      # and a tie is never "decided"


def test_update_inputs():
    for N, D, Kc, empty, stray in K.UPDATE_CASES:
        Z, labels = K.update_case(N, D, Kc, 1000 + N + D, empty, stray)
        n, S, Q = K.update(Z, labels, Kc)
        inside = (labels >= 0) & (labels < Kc)
        assert n.sum() == inside.sum() and (inside.all() != stray)
        if empty is not None:
            assert n[empty] == 0 and not S[empty].any()
        nl, Sl, Ql = K.update(Z, labels, Kc, LD)
        bS, bQ = K.sum_bar(Z, labels, Kc)
        assert np.all(np.abs(S - Sl) <= bS) and np.all(np.abs(Q - Ql) <= bQ)     # NumPy's own sums obey the bar too


def test_emptied_cluster_keeps_its_centre():
    C = np.array([[1.0, 2.0], [5.0, 5.0], [-3.0, 0.0]])
    R = np.array([[1.0, 1.0], [3.0, 1.0], [-3.0, 0.5], [-3.0, -0.5]])
    labels = np.array([0, 0, 2, 2])
    for mom in (K.moments, None):
        if mom is None:
            from eaqhm_amd import convert
            mom = convert.kmeans_moments
        mean, v, sse = mom(C, *K.update(R, labels, 3))
        assert np.array_equal(mean, [[2.0, 1.0], [5.0, 5.0], [-3.0, 0.0]])
        assert np.array_equal(v, [[1.0, 0.0], [0.0, 0.0], [0.0, 0.25]]) and np.array_equal(sse, [2.0, 0.0, 0.5])


def test_split_rule_on_a_hand_made_set():
    """Three clusters: 0 is tight, 1 is wide along column 2, 2 is a single row.  One split (k = 4) takes cluster 1 along
    column 2; two splits (k = 5) take 1 then 0, cluster 2 (n = 1) never."""
    from eaqhm_amd import convert
    R = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0],                                    # cluster 0: v = (0, 1/4, 0)
                  [10.0, 0.0, -4.0], [10.0, 0.0, 4.0], [10.0, 2.0, -4.0], [10.0, 2.0, 4.0],   # cluster 1: v = (0, 1, 16)
                  [-7.0, -7.0, -7.0]])
    labels = np.array([0, 0, 1, 1, 1, 1, 2])
    count, S1, Q = K.update(R, labels, 3)
    C, v, sse = K.moments(np.zeros((3, 3)), count, S1, Q)
    assert np.array_equal(sse, [0.5, 68.0, 0.0])
    assert K.split_choice(count, v, sse, 4) == [(1, 2)] and K.split_choice(count, v, sse, 5) == [(1, 2), (0, 1)]
    assert K.split_choice(count, v, sse, 64) == [(1, 2), (0, 1)]                      # min(K, k - K) = 3, two qualify
    want = np.vstack((C, [[10.0, 1.0, 4.0]], [[0.0, 1.0, 0.0]]))
    want[1, 2], want[0, 1] = -4.0, 0.0
    for fn in (K.split, convert.kmeans_split):
        assert np.array_equal(fn(C, count, v, sse, 5), want)
    tie = np.array([[1.0, 1.0], [1.0, 1.0]])                                          # equal sse, equal v: lowest indices
    assert K.split_choice(np.array([2, 2]), tie, np.array([4.0, 4.0]), 3) == [(0, 0)]
    assert np.array_equal(convert.kmeans_split(np.zeros((2, 2)), np.array([2, 2]), tie, np.array([4.0, 4.0]), 3),
                          [[-1.0, 0.0], [0.0, 0.0], [1.0, 0.0]])


def test_smallest_problems():
    R = np.array([[0.0], [1.0], [4.0]])
    R = R - R.mean()
    one = K.kmeans(R, 1)
    assert one["rounds"] == 1 and not one["labels"].any() and np.allclose(one["centres"], 0.0, atol=1e-15)
    assert np.isclose(one["sse"][0], (R ** 2).sum())
    Z = np.array([[0.0, 0.0], [0.1, 0.0], [5.0, 5.0], [5.0, 5.2]])                     # N = 2 k
    two = K.kmeans(K.rows(Z)[0], 2)
    assert np.array_equal(two["counts"], [2, 2]) and two["labels"][0] == two["labels"][1] != two["labels"][2]


def test_identical_rows_cannot_be_split():
    from eaqhm_amd import convert
    R = np.zeros((8, 3))
    with pytest.raises(np.linalg.LinAlgError, match="split"):
        K.kmeans(R, 2)
    two = np.vstack((np.zeros((4, 2)), np.ones((4, 2)))) - 0.5                         # two points: 2 centres, not 3
    assert np.array_equal(K.kmeans(two, 2)["counts"], [4, 4])
    with pytest.raises(np.linalg.LinAlgError):
        K.kmeans(two, 3)
    count, S1, Q = K.update(two, K.kmeans(two, 2)["labels"], 2)
    C, v, sse = convert.kmeans_moments(np.zeros((2, 2)), count, S1, Q)
    with pytest.raises(np.linalg.LinAlgError, match="cannot be split"):
        convert.kmeans_split(C, count, v, sse, 3)


def test_quality_case():
    """The figures of the module docstring."""
    Z = loop("polytope3")[0]
    axis = float(G.fit(Z, 6, iters=20, tol=0.0)["loglik"][-1])
    km = float(G.fit(Z, 6, iters=20, tol=0.0, init=loop("polytope3")[7]["labels"])["loglik"][-1])
    print("axis start %.6f, k-means start %.6f" % (axis, km))
    assert km > axis + 0.3


# ---- the host side through a NumPy stand-in for the two kernels
class FakeBook:
    """mixture._Codebook with kmeans_ref in place of the library; Z a CPU torch tensor."""
    made = 0

    def __init__(self, torch, c, dev, Z, D, k):
        FakeBook.made += 1
        self.torch, self.D = torch, D
        self.R = Z.numpy()[:, :D]
        self.N = len(self.R)
        self.labels = torch.zeros(self.N, dtype=torch.int32)

    def assign(self, C):
        new = K.assign(self.R, C)
        changed = int((new != self.labels.numpy()).sum())
        self.labels = self.torch.as_tensor(new.astype(np.int32))
        return changed

    def update(self, Kc):
        return K.update(self.R, self.labels.numpy().astype(np.int64), Kc)


class FakeMixture:
    """mixture._Mixture with gmm_ref in place of the library."""

    def __init__(self, Z, zbar, M, device_index):
        import torch
        self.torch, self.c, self.dev = torch, None, "cpu"
        self.N, self.D, self.M = Z.shape[0], Z.shape[1], M
        self.Z = torch.as_tensor(Z - zbar)
        self.gamma = torch.full((self.N, M), float("nan"), dtype=torch.float64)

    def estep(self, mu, W, k):
        _, ll, gamma = G.estep(self.Z.numpy(), mu, W, k)
        self.gamma = self.torch.as_tensor(gamma)
        return self.gamma, ll

    def mstep(self, gamma):
        return G.sufficient(self.Z.numpy(), gamma.numpy())


@pytest.fixture()
def stand_in(monkeypatch, no_device):
    """eaqhm_amd.mixture, where kmeans and gmm_fit look their names up, with the fakes in place of the device classes.
    conversion_train reaches them through gmm_fit; nothing here runs conversion_apply, which makes a _Mixture of its own."""
    import torch
    from eaqhm_amd import mixture
    monkeypatch.setattr(mixture, "_Codebook", FakeBook)
    monkeypatch.setattr(mixture, "_Mixture", FakeMixture)
    monkeypatch.setattr(mixture, "_device", lambda i: (torch, None, "cpu"))
    FakeBook.made = 0
    return mixture


@pytest.mark.parametrize("name", ["polytope3", "corners5"])
def test_host_loop_is_the_model(stand_in, name):
    Z, k, split, scale, R, zbar, sd, f, _ = loop(name)
    out = stand_in.kmeans(Z, k, split=split, scale=scale)
    assert set(out) == {"labels", "centres", "counts", "sse", "rounds"}
    assert np.array_equal(out["labels"], f["labels"]) and out["labels"].dtype == np.int64
    assert np.array_equal(out["counts"], f["counts"]) and out["rounds"] == f["rounds"]
    assert np.array_equal(out["centres"], f["centres"] * sd + zbar) and np.array_equal(out["sse"], f["sse"])
    assert out["centres"].shape == (k, split or Z.shape[1])
    rows, zb, s = stand_in.kmeans_rows(Z, split, scale)
    assert np.array_equal(rows, R) and np.array_equal(zb, zbar) and np.array_equal(s, sd)
    short = stand_in.kmeans(Z, k, split=split, scale=scale, iters=0, split_iters=0)
    assert short["rounds"] == 0 and short["counts"].sum() == len(Z)
    if scale is None:
        assert np.array_equal(stand_in.kmeans_assign(out["centres"], Z), out["labels"])


def test_init_kmeans_reaches_kmeans_and_none_does_not(stand_in, monkeypatch):
    Z = loop("polytope3")[0]
    labels = loop("polytope3")[7]["labels"]
    fit = stand_in.gmm_fit(Z, 6, iters=3, tol=0.0, init="kmeans")
    assert FakeBook.made == 1
    ref = G.fit(Z, 6, iters=3, tol=-1.0, init=labels)
    assert np.allclose(fit["loglik"], ref["loglik"], rtol=0, atol=1e-12) and np.allclose(fit["means"], ref["means"], atol=1e-12)
    seen = []
    real = stand_in.gmm_init_labels
    monkeypatch.setattr(stand_in, "gmm_init_labels", lambda X, M: seen.append(X.shape) or real(X, M))
    FakeBook.made = 0
    for init, calls in ((None, [(600, 2)]), (labels, [])):
        del seen[:]
        fit2 = stand_in.gmm_fit(Z, 6, iters=2, tol=0.0, init=init, split=2)
        assert seen == calls and FakeBook.made == 0 and len(fit2["loglik"]) == 2
    # the split reaches the codebook: with split = 2 it sees two columns
    stand_in.gmm_fit(Z, 4, iters=1, init="kmeans", split=2)
    assert FakeBook.made == 1
    # conversion_train passes the string on, with the x columns as the split
    zero = np.zeros((len(Z), 1))
    got = {}

    def fit_stub(Zj, M, **kw):
        got.update(kw)
        raise KeyError("stop")
    from eaqhm_amd import convert, mapping
    monkeypatch.setattr(mapping, "gmm_fit", fit_stub)
    with pytest.raises(KeyError):
        convert.conversion_train(np.hstack((zero, Z[:, :2])), np.hstack((zero, Z[:, 1:])), 4, init="kmeans")
    assert got["init"] == "kmeans" and got["split"] == 2


def test_empty_final_cluster_is_named(stand_in, monkeypatch):
    Z = loop("polytope3")[0]
    monkeypatch.setattr(stand_in, "kmeans_grow",
                        lambda book, k, **kw: (np.zeros((k, book.D)), np.array([300, 0, 300]), np.zeros(k), 1))
    with pytest.raises(np.linalg.LinAlgError, match="component 1 without a row"):
        stand_in.gmm_fit(Z, 3, init="kmeans")


# ---- every ValueError, before any device work
def test_argument_errors(no_device):
    from eaqhm_amd import (check_conversion_arguments, check_gmm_arguments, check_kmeans_arguments, conversion_train,
                           gmm_fit, kmeans, kmeans_assign)
    Z = np.random.default_rng(0).standard_normal((20, 4))
    got = check_kmeans_arguments(Z.astype(np.float32), 3, 0, 0, 4, "std")
    assert got[0].dtype == np.float64 and got[1:] == (3, 0, 0, 4, "std")
    assert check_kmeans_arguments(Z, 10)[1:] == (10, 20, 2, None, None)                # N = 2 k
    assert check_kmeans_arguments(Z, np.int64(1), 1000, 100, 1)[1:] == (1, 1000, 100, 1, None)
    nan = Z.copy()
    nan[3, 1] = np.nan
    bad = [dict(Z=nan), dict(Z=Z[0]), dict(Z=np.zeros((20, 129))), dict(Z=np.zeros((0, 3))), dict(Z="rows"),
           dict(Z=Z.astype(complex)), dict(k=0), dict(k=65), dict(k=11), dict(k=2.5), dict(k="a"), dict(k=True),
           dict(iters=-1), dict(iters=1001), dict(iters=1.5), dict(split_iters=-1), dict(split_iters=101),
           dict(split_iters="a"), dict(split=0), dict(split=5), dict(split=1.5), dict(scale="var"), dict(scale=1),
           dict(scale=True), dict(scale=b"std")]
    for kw in bad:
        args = dict(dict(Z=Z, k=3), **kw)
        with pytest.raises(ValueError):
            check_kmeans_arguments(**args)
        with pytest.raises(ValueError):
            kmeans(**args)
    with pytest.raises(AssertionError, match="device work"):                           # good arguments reach the device
        kmeans(Z, 3, split=2, scale="std")
    C = Z[:3]
    for centres, rows in ((C, Z[:, :3]), (C[0], Z), (np.zeros((65, 4)), Z), (C, nan), (nan[:5], Z), (C, Z[0]),
                          (np.zeros((0, 4)), Z), (np.zeros((2, 129)), np.zeros((5, 129)))):
        with pytest.raises(ValueError):
            kmeans_assign(centres, rows)
    with pytest.raises(AssertionError, match="device work"):
        kmeans_assign(C, Z)
    assert check_gmm_arguments(Z, 3, init="kmeans")[5] == "kmeans"
    check_conversion_arguments(Z, Z, 3, init="kmeans")
    for init in ("lbg", "", "KMEANS", b"kmeans", 2.5):
        with pytest.raises(ValueError):
            check_gmm_arguments(Z, 3, init=init)
        with pytest.raises(ValueError):
            gmm_fit(Z, 3, init=init)
        with pytest.raises(ValueError):
            conversion_train(Z, Z, 3, init=init)
    with pytest.raises(AssertionError, match="device work"):
        gmm_fit(Z, 3, init="kmeans")


# ---- the binding
KMEANS_ARGUMENT_COUNTS = dict(eaqhm_kmeans_work_len=3, eaqhm_kmeans_assign=10, eaqhm_kmeans_update=11)


def test_symbols():
    import eaqhm_amd  # noqa: F401
    from eaqhm_amd import convert, hip
    assert hip.ABI_VERSION == 6
    common = open(os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc", "eaqhm_common.h")).read()
    assert re.search(r"#define\s+EAQHM_ABI_VERSION\s+6\b", common)
    bound = {name: len(args) for name, _, args in hip.SYMBOLS_KMEANS}
    others = hip.SYMBOLS + hip.SYMBOLS_MLPG + hip.SYMBOLS_GV + hip.SYMBOLS_CEPWARP
    assert not set(bound) & {name for name, _, _ in others}                            # a table of their own
    header = open(os.path.join(ROOT, "include", "eaqhm_kmeans.h")).read()
    assert '#include "eaqhm_kmeans.h"' in open(os.path.join(ROOT, "include", "eaqhm_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(eaqhm_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(bound) == set(KMEANS_ARGUMENT_COUNTS)
    for name, n in KMEANS_ARGUMENT_COUNTS.items():
        assert bound[name] == n, name
        decl = re.search(r"^(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header, re.M)
        assert decl is not None and len(decl.group(1).split(",")) == n, name
    for name in ("kmeans_work_len", "kmeans_assign", "kmeans_update"):
        assert callable(getattr(hip.Context, name))
    lib = hip.load_library()
    assert lib.eaqhm_kmeans_assign(None, None, 1, 1, 1, None, None, 1, None, None) == -1          # EAQHM_EINVAL
    assert lib.eaqhm_kmeans_update(None, None, 1, 1, 1, None, 1, None, None, None, None) == -1
    makefile = open(os.path.join(ROOT, "eaqhm-analysis-and-synthesis-in-python_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*:=.*\beaqhm_kmeans\.hip\b", makefile, re.M)
    assert re.search(r"^HDR\s*:=.*include/eaqhm_kmeans\.h\b", makefile, re.M)
    for N in (1, 511, 512, 513, 65536, 65537, 10 ** 6, 2 ** 31 - 1):
        for D, Kc in ((1, 1), (36, 8), (100, 32), (128, 64)):
            want = -(-N // convert.gmm_chunk_rows(N)) * Kc * (2 * D + 1)
            assert lib.eaqhm_kmeans_work_len(N, D, Kc) == convert.kmeans_work_len(N, D, Kc) == want, (N, D, Kc)
    for N, D, Kc in ((0, 1, 1), (2 ** 31, 1, 1), (1, 0, 1), (1, 129, 1), (1, 1, 0), (1, 1, 65), (-1, 1, 1)):
        assert lib.eaqhm_kmeans_work_len(N, D, Kc) == -1, (N, D, Kc)


def test_exports():
    import eaqhm_amd
    for name in ("kmeans", "kmeans_assign", "check_kmeans_arguments"):
        assert callable(getattr(eaqhm_amd, name))
    from eaqhm_amd import convert
    assert "kmeans(Z, k" in convert.__doc__ and "§12.3" in convert.__doc__


# ---- the CLI
def test_cli_flag(monkeypatch):
    from eaqhm_amd import cli
    train = ["x.wav", "--conversion-train", "t.wav", "--conversion-save", "m.npz"]
    assert cli.parser().parse_args(train).conversion_init is None
    assert cli.conversion_init(cli.parser().parse_args(train)) == {}
    assert cli.conversion_init(cli.parser().parse_args(train + ["--conversion-init", "axis"])) == {}
    a = cli.parser().parse_args(train + ["--conversion-init", "kmeans", "--conversion-span", "2"])
    assert a.conversion_init == "kmeans" and cli.conversion_init(a) == dict(init="kmeans")
    for argv in (["x.wav", "--conversion-init", "kmeans"], ["x.wav", "--conversion-init", "axis"],
                 train + ["--conversion-init", "lbg"], train + ["--conversion-init"],
                 ["x.wav", "--conversion", "m.npz", "--conversion-init", "kmeans"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    assert "--conversion-init" in cli.__doc__


def test_cli_training_passes_the_start_on(tmp_path, monkeypatch):
    from eaqhm_amd import cli, convert, model
    from test_mlpg_cpu import host_dynamic_conversion
    conv, _, _ = host_dynamic_conversion()
    n = 12
    seen = []
    monkeypatch.setattr(model, "model_parameters", lambda det, fs, order=None, lam=5e-4, **kw: dict(
        f0=np.full(n, 100.0), ceps=np.zeros((n, 3)), voiced=np.ones(n, bool), step=80, fs=fs))
    monkeypatch.setattr(cli, "align_other", lambda *a, **k: (np.zeros((n, 3)), np.zeros((n, 2), dtype=np.int64), {}, None))
    monkeypatch.setattr(convert, "conversion_pairs", lambda CA, CB, path, span=None, **k: (np.zeros((n, 6)), np.zeros((n, 6))))
    monkeypatch.setattr(convert, "conversion_train", lambda X, Y, components, **kw: seen.append(kw) or dict(conv))
    out = os.path.join(tmp_path, "m.npz")
    base = ["x.wav", "--conversion-train", "t.wav", "--conversion-save", out, "--conversion-span", "2"]
    for extra, want in (([], None), (["--conversion-init", "axis"], None), (["--conversion-init", "kmeans"], "kmeans")):
        cli.train_conversion(cli.parser().parse_args(base + extra), "male", {}, 16000, {})
        assert seen[-1].get("init") == want and ("init" in seen[-1]) == (want is not None)
