"""The nearest-row search and the non-parallel training on the MI355X (eaqhm_amd.nonparallel -> eaqhm_nn_rows) against
the NumPy model of DESIGN.md §12.5 (tests/nn_ref.py).  Hand-built inputs only; the conditions on the inputs (at most 1 %
of undecided rows, none in the loop, exact ties where ties are meant) are checked on the CPU in
tests/test_nonparallel_cpu.py.

Bars.  Search: the index equals the long-double model's on every decided row (kmeans_ref's docstring derives when a row is
decided); on any other row the device's choice has an exact score within the decision bound of the best
(nn_ref.within_bound); no row is skipped.  Ties are built from small integers, so that every score is exact: the lowest
index wins.  dist2: exactly 0 for equal rows, and within nn_ref.dist2_bar, twice the worst-case rounding error
(D + 2) u dist2 derived in nn_ref's docstring, of the long-double model; its ratio to the model's own
float64-to-long-double difference is recorded.  Placement: the same bits under a permutation of A, after appending rows to A
and on a second launch.  Loop: the same pairs in every round as the float64 model; the trace and the returned map's
fields within 100 x the model's own float64-to-long-double difference, the measured multiples recorded (DESIGN.md §12.5
states them); held-out rms of the returned map at most 0.6 x the identity's."""
import numpy as np
import pytest

import gmm_ref as G
import nn_ref as N
from conftest import record_measurement

pytestmark = pytest.mark.gpu

LD = np.longdouble
CANARY = -0x5A5A5A5A


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


def gpu_nn(A, B, D, launches=1):
    """One or more launches of eaqhm_nn_rows on host arrays A [nA, lda], B [nB, ldb]: [(index, dist2)]; the words behind
    every buffer are checked."""
    from eaqhm_amd import nonparallel
    torch, c, d = ctx()
    (nA, lda), (nB, ldb) = A.shape, B.shape
    words = c.nn_work_len(nA, nB, D)
    assert words == nonparallel.nn_work_len(nA, nB, D) and c.nn_splits(nA, nB) == nonparallel.nn_splits(nA, nB)
    Ad, Bd = torch.as_tensor(np.ascontiguousarray(A), device=d), torch.as_tensor(np.ascontiguousarray(B), device=d)
    out = []
    for _ in range(launches):
        work = torch.full((words + 8,), np.nan, dtype=torch.float64, device=d)
        index = torch.full((nA + 8,), CANARY, dtype=torch.int64, device=d)
        dist2 = torch.full((nA + 8,), np.nan, dtype=torch.float64, device=d)
        c.nn_rows(Ad, nA, lda, Bd, nB, ldb, D, work[:words], index[:nA], dist2[:nA])
        assert np.all(index[nA:].cpu().numpy() == CANARY)
        assert np.all(np.isnan(dist2[nA:].cpu().numpy())) and np.all(np.isnan(work[words:].cpu().numpy()))
        out.append((index[:nA].cpu().numpy(), dist2[:nA].cpu().numpy()))
    return out


# ---- 1. the search
@pytest.mark.parametrize("i", range(len(N.SEARCH_SHAPES)))
def test_search_against_long_double(amd, i):
    """Every shape of nn_ref.SEARCH_SHAPES: NaN in the unused columns where lda, ldb > D, every row checked, dist2 against
    its bar, the same bits on a second launch."""
    A, B = N.search_case(i)
    nA, nB, D = N.SEARCH_SHAPES[i][:3]
    (idx, d2), (idx2, d2b) = gpu_nn(A, B, D, launches=2)
    a, b = A[:, :D], B[:, :D]
    want = N.nearest(a, b, LD)
    ok = N.decided(a, b)
    exact = N.dist2(a, b, idx, LD)
    err = np.abs(d2.astype(LD) - exact).astype(np.float64)
    own = np.abs(N.dist2(a, b, idx).astype(LD) - exact).astype(np.float64)
    bar = N.dist2_bar(a, b, idx)
    ratio = float(err.max() / own.max()) if own.max() > 0 else None
    print("search %s: %d of %d rows decided, %d indices differ, dist2 error / bar %.3g, / the model's own %s"
          % (N.SEARCH_SHAPES[i], ok.sum(), nA, (idx != want).sum(), float((err / np.maximum(bar, 1e-300)).max()), ratio))
    record_measurement("nn_search_%d" % i, shape=list(N.SEARCH_SHAPES[i][:3]), decided=int(ok.sum()),
                       dist2_err_over_bar=float((err / np.maximum(bar, 1e-300)).max()), dist2_err_over_model=ratio)
    assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < nB
    assert np.array_equal(idx[ok], want[ok])
    assert np.all(N.within_bound(a, b, idx))                             # the rows that are not decided as well
    assert np.all(d2 >= 0) and np.all(err <= bar)
    assert np.array_equal(idx2, idx) and np.array_equal(d2b, d2)


def test_ties_take_the_lowest_index(amd):
    """Identical rows of B within a panel, across a panel boundary and across a split boundary, and two different rows at
    the same distance in different splits; a row of A equal to a row of B has dist2 exactly 0."""
    A, B, want = N.tie_case()
    s = N.scores(A, B)                                                  # exact in float64: integers far below 2^53
    exact = np.argmin(s, axis=1)
    tied = (s == s.min(axis=1)[:, None]).sum(axis=1) > 1
    assert all(exact[i] == j for i, j in want.items()) and tied[:4].all()
    (idx, d2), = gpu_nn(A, B, 6)
    assert np.array_equal(idx, exact)
    assert np.array_equal(d2, N.dist2(A, B, exact)) and np.all(d2[:3] == 0.0) and d2[3] == 4.0


def test_equal_rows_have_distance_zero(amd):
    A, B = N.search_case(9)                                             # 65 x 8200 x 36, three splits
    D = 36
    pick = np.random.default_rng(4).integers(0, len(B), size=len(A))
    A = np.array(A)
    A[:, :D] = B[pick, :D]
    (idx, d2), = gpu_nn(A, B, D)
    assert np.array_equal(idx, pick) and np.all(d2 == 0.0)


# ---- 2. placement
def test_placement_does_not_matter(amd):
    """Permuting A permutes index and dist2 bit for bit; appending rows to A changes nothing for the old rows (130 rows in
    three blocks against 4160 rows in two splits)."""
    A, B = N.search_case(8)
    D = 5
    (idx, d2), = gpu_nn(A, B, D)
    perm = np.random.default_rng(6).permutation(len(A))
    (idx_p, d2_p), = gpu_nn(A[perm], B, D)
    assert np.array_equal(idx_p, idx[perm]) and np.array_equal(d2_p, d2[perm])
    for n in (1, 63, 65):
        (idx_n, d2_n), = gpu_nn(A[:n], B, D)
        assert np.array_equal(idx_n, idx[:n]) and np.array_equal(d2_n, d2[:n]), n


# ---- 3. errors
def test_bad_arguments_launch_nothing(amd):
    torch, c, d = ctx()
    A = torch.zeros((8, 4), dtype=torch.float64, device=d)
    B = torch.ones((9, 4), dtype=torch.float64, device=d)
    work = torch.full((64,), 7.0, dtype=torch.float64, device=d)
    index = torch.full((8,), CANARY, dtype=torch.int64, device=d)
    dist2 = torch.full((8,), 7.0, dtype=torch.float64, device=d)
    a, b, w, i, s = (t.data_ptr() for t in (A, B, work, index, dist2))
    good = [a, 8, 4, b, 9, 4, 4, w, i, s]
    assert c.nn_work_len(8, 9, 4) <= 64
    bad = [{1: 0}, {4: 0}, {1: 2 ** 31}, {4: 2 ** 31}, {1: -1}, {6: 0}, {6: 129}, {6: 5}, {2: 3}, {5: 3}, {0: None}, {3: None},
           {7: None}, {8: None}, {9: None}]
    for change in bad:
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert c.lib.eaqhm_nn_rows(c.h, *args) == -1, change            # EAQHM_EINVAL
        assert b"eaqhm_nn_rows" in c.lib.eaqhm_last_error(c.h)
    assert b"2^31" in c.lib.eaqhm_last_error(c.h) or b"bad argument" in c.lib.eaqhm_last_error(c.h)
    assert c.lib.eaqhm_nn_rows(None, *good) == -1
    torch.cuda.synchronize()
    assert np.all(index.cpu().numpy() == CANARY) and np.all(dist2.cpu().numpy() == 7.0) and np.all(work.cpu().numpy() == 7.0)
    with pytest.raises(RuntimeError, match="1 <= nA, nB < 2\\^31, 1 <= D <= 128"):
        c.nn_rows(A, 8, 4, B, 9, 4, 129, work, index, dist2)
    c.nn_rows(A, 8, 4, B, 9, 4, 4, work, index, dist2)                  # and the good call runs
    assert np.all(index.cpu().numpy() == 0) and np.all(dist2.cpu().numpy() == 4.0)


# ---- 4. the loop
_LOOP = {}


def loop_case():
    """The quality case, the model in both precisions and the device's run, once."""
    if not _LOOP:
        from eaqhm_amd import nonparallel
        S = N.inca_set()
        _LOOP.update(S=S, f=N.loop(S["X"], S["Y"], S["components"]), g=N.loop(S["X"], S["Y"], S["components"], dtype=LD))
        rounds, real = [], nonparallel.nonparallel_pairs
        nonparallel.nonparallel_pairs = lambda p, q=None: rounds.append(real(p, q)) or rounds[-1]
        try:
            conv, info = nonparallel.conversion_train_nonparallel(S["X"], S["Y"], S["components"], level=True)
        finally:
            nonparallel.nonparallel_pairs = real
        _LOOP.update(conv=conv, info=info, rounds=rounds)
    return _LOOP


def test_loop_pairs_and_trace(amd):
    L = loop_case()
    f, g, info = L["f"], L["g"], L["info"]
    assert info["rounds"] == len(f["fits"]) == len(L["rounds"]) and info["best"] == f["best"]
    for r, (got, want) in enumerate(zip(L["rounds"], f["pairs"])):
        assert np.array_equal(got, want), r                               # the same pairs in every round
    pr = f["pairs"][f["best"] - 1]
    assert np.array_equal(info["ix"], pr[:, 0]) and np.array_equal(info["iy"], pr[:, 1])
    model = float(np.abs(f["trace"].astype(LD) - g["trace"]).max())
    err = float(np.abs(info["trace"] - f["trace"]).max())
    print("loop trace: |gpu - model| %.3g, model f64 - long double %.3g, multiple %.3g" % (err, model, err / model))
    print("trace", " ".join("%.4f" % t for t in info["trace"]))
    record_measurement("nn_loop_trace", err=err, model=model, multiple=err / model, trace=[float(t) for t in info["trace"]])
    assert len(info["trace"]) == len(f["trace"]) and err <= 100.0 * model


def test_loop_map_against_the_model(amd):
    L = loop_case()
    f, g, conv = L["f"], L["g"], L["conv"]
    b, dx = f["best"] - 1, 3
    multiples = {}
    fields = []
    for fit in (f["fits"][b], g["fits"][b]):
        A, bb, _, _ = G.conversion(fit["weights"], fit["means"] - fit["zbar"].astype(fit["means"].dtype), fit["covs"], dx)
        fields.append(dict(loglik=fit["loglik"], weights=fit["weights"], means=fit["means"], covs=fit["covs"], A=A, b=bb))
    assert len(conv["loglik"]) == len(fields[0]["loglik"]) == len(fields[1]["loglik"])
    for key in ("loglik", "weights", "means", "covs", "A", "b"):
        model = float(np.abs(fields[0][key].astype(LD) - fields[1][key]).max())
        err = float(np.abs(conv[key] - fields[0][key]).max())
        multiples[key] = err / model
        print("loop map %s: |gpu - model| %.3g, model f64 - long double %.3g, multiple %.3g" % (key, err, model, err / model))
    record_measurement("nn_loop_map", **multiples)
    for key, m in multiples.items():
        assert m <= 100.0, key


def test_loop_quality_and_use(amd):
    """Held-out rms at most 0.6 x the identity's; conversion_apply takes the map; a dynamic map from the pairs is valid."""
    from eaqhm_amd import convert
    L = loop_case()
    S, conv, info = L["S"], L["conv"], L["info"]
    convert.check_conversion(conv)
    assert "span" not in conv and bool(conv["level"]) and int(conv["dx"]) == 3
    out = convert.conversion_apply(conv, S["Xh"])
    ident, held = N.rms(S["Xh"], S["Yh"]), N.rms(out, S["Yh"])
    print("held-out rms %.3f, identity %.3f, ratio %.3f" % (held, ident, held / ident))
    record_measurement("nn_loop_quality", held=held, identity=ident)
    assert out.shape == S["Yh"].shape and held <= 0.6 * ident
    X2, Y2 = convert.dynamic_rows(S["X"], 2)[info["ix"]], convert.dynamic_rows(S["Y"], 2)[info["iy"]]
    dyn = convert.conversion_train(X2, Y2, S["components"], level=True, span=2)
    checked = convert.check_conversion(dyn)
    assert checked["span"] == 2 and checked["dx"] == 6 and int(dyn["n"]) == len(info["ix"])


def test_nearest_rows_is_the_kernel(amd):
    from eaqhm_amd import nonparallel
    A, B = N.search_case(8)
    idx, d2 = nonparallel.nearest_rows(A[:, :5], B[:, :5])
    (want, d2w), = gpu_nn(A, B, 5)
    assert np.array_equal(idx, want) and np.array_equal(d2, d2w) and idx.dtype == np.int64 and d2.dtype == np.float64
