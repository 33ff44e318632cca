"""The k-means codebook on the MI355X (convert.kmeans / kmeans_assign / gmm_fit(init="kmeans") -> eaqhm_kmeans_assign,
eaqhm_kmeans_update) against the NumPy model of DESIGN.md §12.3 (tests/kmeans_ref.py).  Hand-built inputs only; the
conditions on the inputs (no undecided row, exact ties where ties are meant) are checked on the CPU in
tests/test_kmeans_cpu.py.

Bars.  Assignment: exact equality with the long-double model on every decided row (kmeans_ref's docstring derives when a
row is decided), and the lowest index on exact ties, which are built from small integers so that every score is exact.
Update: counts exact; S1 and Q within kmeans_ref.sum_bar, twice the worst-case rounding error 2 n_m u sum |x| of a sum of
the n_m terms of a cluster, of the long-double model.  Loop: labels equal to the float64 model's, centres within 100 x the model's own
float64-to-long-double difference.  gmm_fit(init="kmeans"): the same 100 x rule against gmm_ref.fit started from the
model's labels.  init=None: the sha256 of the commit before (tests/kmeans_parent_cases.py)."""
import json

import numpy as np
import pytest

import gmm_ref as G
import kmeans_parent_cases as P
import kmeans_ref as K
from conftest import record_measurement

pytestmark = pytest.mark.gpu

LD = np.longdouble
CANARY = 0x5A5A5A5A


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


def gpu_assign(Z, D, C, before, launches=1):
    """One or more launches of eaqhm_kmeans_assign on host arrays: [(labels, changed per block)], and the canaries."""
    torch, c, d = ctx()
    N, ldz = Z.shape
    K = len(C)
    blocks = -(-N // 64)
    Zd = torch.as_tensor(np.ascontiguousarray(Z), device=d)
    Cd = torch.as_tensor(np.ascontiguousarray(C, dtype=np.float64), device=d)
    gd = torch.as_tensor((np.asarray(C, dtype=np.float64) ** 2).sum(axis=1), device=d)
    lab = torch.full((N + 8,), CANARY, dtype=torch.int32, device=d)
    lab[:N] = torch.as_tensor(np.asarray(before, dtype=np.int32), device=d)
    chg = torch.full((blocks + 8,), CANARY, dtype=torch.int32, device=d)
    out = []
    for _ in range(launches):
        c.kmeans_assign(Zd, N, ldz, D, Cd, gd, K, lab[:N], chg[:blocks])
        out.append((lab[:N].cpu().numpy().astype(np.int64), chg[:blocks].cpu().numpy().astype(np.int64)))
    assert np.all(lab[N:].cpu().numpy() == CANARY) and np.all(chg[blocks:].cpu().numpy() == CANARY)
    return out


def gpu_update(Z, D, labels, K, launches=1):
    torch, c, d = ctx()
    N, ldz = Z.shape
    words = c.kmeans_work_len(N, D, K)
    from eaqhm_amd import convert
    assert words == convert.kmeans_work_len(N, D, K)
    Zd = torch.as_tensor(np.ascontiguousarray(Z), device=d)
    ld = torch.as_tensor(np.asarray(labels, dtype=np.int32), device=d)
    out = []
    for _ in range(launches):
        work = torch.full((words + 8,), np.nan, dtype=torch.float64, device=d)
        count = torch.full((K + 8,), -7, dtype=torch.int64, device=d)
        S1 = torch.full((K * D + 8,), np.nan, dtype=torch.float64, device=d)
        Q = torch.full((K * D + 8,), np.nan, dtype=torch.float64, device=d)
        c.kmeans_update(Zd, N, ldz, D, ld, K, work[:words], count[:K], S1[:K * D], Q[:K * D])
        assert np.all(count[K:].cpu().numpy() == -7)
        for buf, n in ((work, words), (S1, K * D), (Q, K * D)):
            assert np.all(np.isnan(buf[n:].cpu().numpy()))
        out.append((count[:K].cpu().numpy(), S1[:K * D].cpu().numpy().reshape(K, D), Q[:K * D].cpu().numpy().reshape(K, D)))
    return out


# ---- 1. the assignment
@pytest.mark.parametrize("i", range(len(K.ASSIGN_SHAPES)))
def test_assign_against_long_double(amd, i):
    """Every shape of kmeans_ref.ASSIGN_SHAPES: NaN in the unused columns where ldz > D, labels in and out, the counts of
    moved rows, the words behind both outputs, the same bits on a second launch."""
    Z, C = K.assign_case(i)
    N, D, Kc = Z.shape[0], C.shape[1], len(C)
    before = np.random.default_rng(i).integers(0, Kc, size=N)
    (lab, chg), (lab2, chg2) = gpu_assign(Z, D, C, before, launches=2)
    want = K.assign(Z[:, :D], C, LD)
    ok = K.decided(Z[:, :D], C)
    print("assign %s: %d of %d rows decided, %d labels differ" % (K.ASSIGN_SHAPES[i], ok.sum(), N, (lab != want).sum()))
    assert lab.min() >= 0 and lab.max() < Kc
    assert np.array_equal(lab[ok], want[ok])
    moved = (lab != before).astype(np.int64)
    assert np.array_equal(chg, np.add.reduceat(moved, np.arange(0, N, 64)))
    assert np.array_equal(lab2, lab) and not chg2.any()


def test_assign_ties_take_the_lowest_index(amd):
    Z, C = K.tie_case()
    s = (C * C).sum(axis=1)[None, :] - 2 * Z @ C.T                  # exact in float64: integers far below 2^53
    want = np.argmin(s, axis=1)
    tied = (s == s.min(axis=1)[:, None]).sum(axis=1) > 1
    assert tied[0] and want[0] == 38 and want[1 + 20] == 3 and want[1 + 37] == 5 and tied.sum() >= 5
    (lab, _), = gpu_assign(Z, 20, C, np.zeros(len(Z)))
    assert np.array_equal(lab, want)


# ---- 2. the update
@pytest.mark.parametrize("N,D,Kc,empty,stray", K.UPDATE_CASES)
def test_update_against_long_double(amd, N, D, Kc, empty, stray):
    from eaqhm_amd import convert
    assert convert.gmm_chunk_rows(N) == 512
    Z, labels = K.update_case(N, D, Kc, 1000 + N + D, empty, stray)
    (count, S1, Q), (count2, S1b, Qb) = gpu_update(Z, D, labels, Kc, launches=2)
    n, S, QQ = K.update(Z, labels, Kc, LD)
    bS, bQ = K.sum_bar(Z, labels, Kc)
    assert np.array_equal(count, n)
    if empty is not None:
        assert count[empty] == 0 and not S1[empty].any() and not Q[empty].any()
    eS, eQ = np.abs(S1 - S).astype(np.float64), np.abs(Q - QQ).astype(np.float64)
    worst = max(float((eS / np.where(bS > 0, bS, 1)).max()), float((eQ / np.where(bQ > 0, bQ, 1)).max()))
    print("update N=%d D=%d K=%d: worst error / bar %.3g" % (N, D, Kc, worst))
    record_measurement("kmeans_update_%d_%d_%d" % (N, D, Kc), worst_err_over_bar=worst)
    assert np.all(eS <= bS) and np.all(eQ <= bQ)
    assert np.array_equal(count2, count) and np.array_equal(S1b, S1) and np.array_equal(Qb, Q)


def test_update_reads_only_the_first_columns(amd):
    Z, labels = K.update_case(600, 6, 4, 3)
    wide = np.full((600, 9), np.nan)
    wide[:, :6] = Z
    (a,), (b,) = gpu_update(Z, 6, labels, 4), gpu_update(wide, 6, labels, 4)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 3. the loop
_LOOP = {}


def loop_reference(name):
    if name not in _LOOP:
        Z, k, split, scale = K.loop_case(name)
        R, zbar, sd = K.rows(Z, split, scale)
        _LOOP[name] = (Z, k, split, scale, R, zbar, sd, K.kmeans(R, k), K.kmeans(R, k, dtype=LD))
    return _LOOP[name]


@pytest.mark.parametrize("name", ["polytope3", "corners5"])
def test_loop_against_the_model(amd, name):
    Z, k, split, scale, R, zbar, sd, f, g = loop_reference(name)
    for C, _ in f["assigns"]:                                       # the model's labels are decided at every round
        assert K.decided(R, C).all()
    out = amd.kmeans(Z, k, split=split, scale=scale)
    assert out["labels"].dtype == np.int64 and out["counts"].dtype == np.int64
    assert np.array_equal(out["labels"], f["labels"])
    assert np.array_equal(out["counts"], f["counts"]) and out["rounds"] == f["rounds"]
    model = float(np.abs((f["centres"] * sd + zbar).astype(LD) - (g["centres"] * sd.astype(LD) + zbar.astype(LD))).max())
    err = float(np.abs(out["centres"] - (f["centres"] * sd + zbar)).max())             # in Z's coordinates, as returned
    print("kmeans %s: |gpu - model| %.3g, model f64 - long double %.3g, %d rounds" % (name, err, model, out["rounds"]))
    record_measurement("kmeans_loop_%s" % name, err=err, model_diff=model, rounds=out["rounds"])
    assert err <= 100.0 * model
    assert np.abs(out["sse"] - f["sse"]).max() <= 1e-9 * f["sse"].max()
    again = amd.kmeans_assign(out["centres"], Z[:, :split] if split else Z) if scale is None else None
    if again is not None:
        assert np.array_equal(again, out["labels"])


# ---- 4. the mixture started from the codebook
def test_gmm_fit_from_kmeans(amd):
    Z = loop_reference("polytope3")[0]
    labels = loop_reference("polytope3")[7]["labels"]
    f = G.fit(Z, 6, iters=6, tol=-1.0, init=labels)
    g = G.fit(Z, 6, iters=6, tol=-1.0, init=labels, dtype=LD)
    fit = amd.gmm_fit(Z, 6, iters=6, tol=0.0, init="kmeans")
    assert len(fit["loglik"]) == 6
    for key in ("loglik", "weights", "means", "covs"):
        model = float(np.abs(f[key].astype(LD) - g[key]).max())
        err = float(np.abs(fit[key] - f[key]).max())
        print("gmm_fit(init=kmeans) %s: |gpu - model| %.3g, model f64 - long double %.3g" % (key, err, model))
        record_measurement("kmeans_gmm_%s" % key, err=err, model_diff=model)
        assert err <= 100.0 * model, (key, err, model)


def test_kmeans_start_ends_above_the_axis_start(amd):
    """The quality case: 20 rounds, tol = 0."""
    Z = loop_reference("polytope3")[0]
    axis = amd.gmm_fit(Z, 6, iters=20, tol=0.0)["loglik"][-1]
    km = amd.gmm_fit(Z, 6, iters=20, tol=0.0, init="kmeans")["loglik"][-1]
    print("mean log-likelihood after 20 rounds: axis start %.6f, k-means start %.6f" % (axis, km))
    record_measurement("kmeans_quality_polytope3", axis=float(axis), kmeans=float(km))
    assert km > axis
    zero = np.zeros((len(Z), 1))                                     # conversion_train passes the string on
    Y = np.hstack((zero, Z[:, 2:], Z[:, :1] + 0.3 * np.random.default_rng(2).standard_normal((len(Z), 1))))
    a = amd.conversion_train(np.hstack((zero, Z[:, :2])), Y, 4, iters=5, tol=0.0, init="kmeans")
    assert len(a["loglik"]) == 5 and np.all(np.isfinite(a["A"]))


def test_bad_sizes_are_error_codes(amd):
    torch, c, d = ctx()
    from eaqhm_amd import hip
    z = torch.zeros((4, 4), dtype=torch.float64, device=d)
    lab = torch.zeros(4, dtype=torch.int32, device=d)
    cnt = torch.zeros(4, dtype=torch.int64, device=d)
    for N, ldz, D, Kc in ((0, 4, 4, 1), (4, 3, 4, 1), (4, 4, 0, 1), (4, 129, 129, 1), (4, 4, 4, 0), (4, 4, 4, 65),
                          (2 ** 31, 4, 4, 1)):
        with pytest.raises(RuntimeError):
            c.kmeans_assign(z, N, ldz, D, z, z, Kc, lab, lab)
        with pytest.raises(RuntimeError):
            c.kmeans_update(z, N, ldz, D, lab, Kc, z, cnt, z, z)
    assert hip.ABI_VERSION == 6


# ---- 5. init=None is the commit before, bit for bit
@pytest.mark.parametrize("name", ["fit", "train_span2"])
def test_default_start_is_the_parent(amd, name):
    with open(P.FIXTURE) as fh:
        doc = json.load(fh)
    assert P.digest(P.cases()[name](amd)) == doc["cases"][name]
