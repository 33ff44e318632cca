"""Spectral conversion learned from aligned cepstral rows: a joint-density Gaussian mixture (not in the reference), the
trajectory conversion on top of it, and the one import point of the whole conversion layer.

    gmm_fit(Z, components, *, iters=20, tol=1e-5, floor=1e-6, init=None, split=None, device_index=0)
        -> dict(weights[M], means[M, D], covs[M, D, D], zbar[D], phi[D], loglik[n_E_steps], n)
    gmm_posteriors(gmm, Z, *, device_index=0) -> (gamma[N, M], ll[N])
    conversion_pairs(CA, CB, path, span=None) -> (X, Y): the rows a model_align path pairs, empty rows dropped; with a
        span the dynamic rows [c | delta c] of both sides
    conversion_train(X, Y, components=8, *, level=False, iters=20, tol=1e-5, floor=1e-6, init=None, span=None, gv=None,
                     device_index=0)
        -> flat dict of arrays (np.savez): the gmm fields + dx, dy, level, A[M, dy, dx], b[M, dy], Wx[M, dx, dx], kx[M];
        with a span also span and py[M, dy], and dx, dy count the delta columns; with gv also gv_mean, gv_prec[dy / 2]
    conversion_apply(conv, C, *, device_index=0) -> float64[n, dy_cols] in model_cepstrum's layout (a static map)
    dynamic_rows(C, span=2, *, device_index=0) -> float64[n, 2 (P + 1)]: [c | delta c] over the runs of non-empty rows
    conversion_trajectory(conv, C, *, gv=None, gv_weight=1.0, gv_iters=30, trace=False, device_index=0)
        -> float64[n, Q + 1]: the most likely trajectory under a dynamic map, with the global-variance term when the map
        or `gv` carries its statistics; with trace=True also the objective float64[gv_iters + 1, dys]
    conversion_trajectory_em(conv, C, *, em_iters=4, em_tol=0.0, em_trace=False, gv=None, gv_weight=1.0, gv_iters=30,
                             trace=False, device_index=0)
        -> the same after `em_iters` EM refinements of the mixture sequence (reached as eaqhm_amd.convert.
        conversion_trajectory_em); with em_trace=True also the mean log-likelihood float64[iterations + 1]
    global_variance(C, level=False) -> float64[cols]: the variance of each mapped static column over the non-empty rows
    gv_statistics(utterances, *, level=False, rel_std=None) -> dict(gv_mean[dys], gv_prec[dys]) for conversion_train(gv=)
    f0_statistics(f0, voiced) -> (mean, std) of ln f0 over the voiced instants
    pitch_conversion_contour(f0, voiced, src_stats, tgt_stats) -> pitch_scale contour float64[n]
    kmeans(Z, k, *, iters=20, split_iters=2, split=None, scale=None, device_index=0)
        -> dict(labels int64[N], centres[k, D'], counts int64[k], sse[k], rounds): a codebook grown by splitting (LBG)
    kmeans_assign(centres, Z, *, device_index=0) -> int64[N]: the nearest centre of each row
    check_gmm_arguments, check_conversion_arguments, check_conversion, check_gv_arguments, check_kmeans_arguments,
    check_em_arguments: validation, no device work

The definitions are DESIGN.md §12 (the mixture and the map), §12.1 (delta rows and the most likely trajectory), §12.2
(the global-variance term), §12.3 (the k-means codebook) and §12.4 (the EM refinement of the mixture sequence).  What is
defined here is the trajectory (eaqhm_mlpg_solve, eaqhm_mlpg_estep, eaqhm_gv_ascend in libeaqhm_hip.so; there is no CPU
path) and the ln-f0 statistics, which are host only.  It sits on top of three modules, which follow args, records,
cepstrum and align and each import only from the ones before them:

    mixture   rows in, clusters out: the k-means codebook and the Gaussian mixture, their chunk rules and host algebra
    dynamics  delta rows and global-variance statistics; the size mirrors of the trajectory's work buffers
    mapping   the conversion map: pair, train, check, apply

mapping follows dynamics because a dynamic map is checked and trained on delta rows; the trajectory starts from a
checked map.  None of them imports noise or model.  Every name of theirs is imported here by name, so
`from eaqhm_amd.convert import X` reaches all of them; cli and nonparallel resolve the public functions through this
module at call time.
"""
import math

import numpy as np

from .align import _path  # noqa: F401
from .args import SCALE_RANGE, _integer, _numeric_1d, _real, _rows  # noqa: F401
from .cepstrum import CEPSTRUM_MAX_ORDER, _cepstrum_rows, check_cepstrum_warp  # noqa: F401
from .records import _agree, _device  # noqa: F401
from .mixture import (GMM_CHUNK_MIN, GMM_CHUNKS_MAX, GMM_FLOOR_RANGE, GMM_MAX_COLUMNS, GMM_MAX_COMPONENTS,  # noqa: F401
                      GMM_MAX_ITERS, GMM_MAX_SIDE, KMEANS_MAX_CENTRES, KMEANS_MAX_ITERS, KMEANS_MAX_SPLIT_ITERS,
                      KMEANS_START, _Codebook, _field, _kmeans_responsibilities, _Mixture, check_gmm,
                      check_gmm_arguments, check_kmeans_arguments, gmm_centre, gmm_chunk_rows,
                      gmm_estep_parameters, gmm_finish_mstep, gmm_fit, gmm_init_labels, gmm_posteriors,
                      gmm_work_len, kmeans, kmeans_assign, kmeans_grow, kmeans_moments, kmeans_rows,
                      kmeans_split, kmeans_work_len)
from .dynamics import (DELTA_SPAN_RANGE, GV_CHUNK_MIN, GV_CHUNKS_MAX, GV_REL_STD_MAX, _dynamic_columns,  # noqa: F401
                       _gv_fields, check_span, delta_runs, dynamic_rows, global_variance, gv_chunk_rows,
                       gv_statistics, gv_work_len, mlpg_work_len)
from .mapping import (_CONVERSION_FIELDS, _has, _nonempty_rows, _put_rows, check_conversion,  # noqa: F401
                      check_conversion_arguments, conversion_apply, conversion_pairs, conversion_train,
                      gmm_conditional_precisions, gmm_conversion_parameters)

GV_WEIGHT_RANGE = (1e-6, 1e6)
GV_MAX_ITERS = 10000
EM_MAX_ITERS = 100         # refinements of the mixture sequence at most


def check_gv_arguments(conv, gv=None, gv_weight=1.0, gv_iters=30, trace=False):
    """Validates the global-variance arguments of conversion_trajectory against a validated dynamic map (check_conversion's
    result; no device work): returns (stats, gv_weight, gv_iters, trace), stats dict(gv_mean, gv_prec) float64[dys] or
    None when the ascent does not run (gv=False, or gv=None with a map that has no statistics)."""
    if "span" not in conv:
        raise ValueError("the global-variance term needs a dynamic map (span)")
    if gv is None:
        stats = {k: conv[k] for k in ("gv_mean", "gv_prec")} if "gv_mean" in conv else None
    elif isinstance(gv, (bool, np.bool_)):
        if gv:
            raise ValueError("gv must be None (the map's statistics), False or a gv_statistics dict")
        stats = None
    else:
        stats = _gv_fields(gv, conv["dy"] // 2, "gv")
    gv_weight = _real(gv_weight, "gv_weight", *GV_WEIGHT_RANGE)
    gv_iters = _integer(gv_iters, "gv_iters")
    if not 0 <= gv_iters <= GV_MAX_ITERS:
        raise ValueError("gv_iters must be in [0, %d], got %d" % (GV_MAX_ITERS, gv_iters))
    if not isinstance(trace, (bool, np.bool_)):
        raise ValueError("trace must be True or False")
    if trace and stats is None:
        raise ValueError("trace=True needs the global-variance term: a map with gv_mean and gv_prec, or gv=")
    return stats, gv_weight, gv_iters, bool(trace)


def check_em_arguments(em_iters=4, em_tol=0.0, em_trace=False):
    """Validates the refinement arguments of conversion_trajectory_em (no device work): returns (em_iters, em_tol,
    em_trace), em_iters an int in [0, 100], em_tol a finite float >= 0, em_trace a bool."""
    em_iters = _integer(em_iters, "em_iters")
    if not 0 <= em_iters <= EM_MAX_ITERS:
        raise ValueError("em_iters must be in [0, %d], got %d" % (EM_MAX_ITERS, em_iters))
    if isinstance(em_tol, (bool, np.bool_)):
        raise ValueError("em_tol must be a number")
    em_tol = _real(em_tol, "em_tol", 0.0, np.inf)
    if not np.isfinite(em_tol):
        raise ValueError("em_tol must be finite")
    if not isinstance(em_trace, (bool, np.bool_)):
        raise ValueError("em_trace must be True or False")
    return em_iters, em_tol, bool(em_trace)


def conversion_trajectory(conv, C, *, gv=None, gv_weight=1.0, gv_iters=30, trace=False, device_index=0):
    """Converts cepstral rows `C` float64[n, dx_cols] (model_cepstrum's layout) with a dynamic map, conversion_train(span=)'s,
    to the trajectory that is most likely under the static and the delta statistics together (Toda,
    Black & Tokuda 2007, the posterior-weighted initial estimate).  With X_t = [x_t | delta x_t], gamma the posteriors of
    the marginal mixture on X, P_t = sum_m gamma_tm py_m and r_t = sum_m gamma_tm py_m (b_m + A_m X_t) (un-centred), every
    run of non-empty rows and every static column d solves (diag(P^s) + W^T diag(P^D) W) y = r^s + W^T r^D, W the run's
    delta matrix.  Nothing couples across an empty row; an empty row comes back empty; with level=False column 0 is the
    source row's.  Returns float64[n, dy_cols], accepted wherever conversion_apply's result is.
    The global-variance term follows when there are statistics for it: gv=None takes the map's gv_mean
    and gv_prec if it has them, gv=False never does, a gv_statistics dict overrides the map.  From the trajectory above,
    scaled per column to the variance gv_mean, `gv_iters` sweeps (0 to 10000; 0 returns the scaled start) climb the
    likelihood joined with the prior of precision `gv_weight` gv_prec (gv_weight in [1e-6, 1e6]) on each column's
    variance over all non-empty rows.  A column that is constant, or an utterance of one non-empty row, stays as it is.
    trace=True returns (rows, float64[gv_iters + 1, dys]), the objective of every column before each sweep and after the
    last."""
    v = check_conversion(conv)
    if "span" not in v:
        raise ValueError("this conversion is a static map (no span): use conversion_apply")
    stats, gv_weight, gv_iters, trace = check_gv_arguments(v, gv, gv_weight, gv_iters, trace)
    out, objective, _ = _trajectory(v, C, stats, gv_weight, gv_iters, trace, device_index)
    return (out, objective) if trace else out


def conversion_trajectory_em(conv, C, *, em_iters=4, em_tol=0.0, em_trace=False, gv=None, gv_weight=1.0, gv_iters=30,
                             trace=False, device_index=0):
    """conversion_trajectory followed by the EM refinement of the mixture sequence (Toda, Black & Tokuda
    2007): conversion_trajectory's estimate y^(0) takes the component posteriors from the source rows alone, pi_tm =
    p(m | X_t).  Under the model the map implies, p(Y_t | X_t) = sum_m pi_tm N(Y_t; b_m + A_m X_t, diag(1 / py_m)) with
    Y_t(y) = [y_t | (W y)_t], each of `em_iters` iterations (0 to 100) revises the posteriors in the light of the
    trajectory, gamma_tm proportional to pi_tm N(Y_t(y^(i)); ..) (eaqhm_mlpg_estep), and solves conversion_trajectory's
    systems again with P and r formed from them: the exact maximiser of EM's auxiliary function, so the log-likelihood
    sum_t ln p(Y_t(y) | X_t) does not fall.  em_iters=0 is conversion_trajectory's result bit for bit.  The default of 4 is
    a stated choice, not a tuned one: on the cases of DESIGN.md §12.4 the gain falls by about a factor of ten per
    iteration.  With em_tol=0 all iterations run and nothing is read back between them; with em_tol > 0 the mean of the
    rows' log-likelihoods is formed on the host after every E-step, and the loop stops, keeping the trajectory that E-step
    scored, once the mean rose by less than em_tol over the previous iteration's.  The global-variance term (gv,
    gv_weight, gv_iters, trace: conversion_trajectory's) then starts from the last P, r and y; the posteriors stay fixed
    during the ascent.  Empty rows, level=False and the layout of `C` are conversion_trajectory's.  em_trace=True also
    returns float64[k + 1], the mean log-likelihood of y^(0) .. y^(k), k the iterations done (one more E-step at the end;
    a single 0 without a non-empty row).  Returns rows, then the objective if trace, then the log-likelihoods if
    em_trace.  A static map is a ValueError naming conversion_apply."""
    v = check_conversion(conv)
    if "span" not in v:
        raise ValueError("this conversion is a static map (no span): use conversion_apply")
    stats, gv_weight, gv_iters, trace = check_gv_arguments(v, gv, gv_weight, gv_iters, trace)
    em_iters, em_tol, em_trace = check_em_arguments(em_iters, em_tol, em_trace)
    out, objective, loglik = _trajectory(v, C, stats, gv_weight, gv_iters, trace, device_index,
                                         dict(iters=em_iters, tol=em_tol, trace=em_trace))
    result = (out,) + ((objective,) if trace else ()) + ((loglik,) if em_trace else ())
    return result if len(result) > 1 else out


def _trajectory(v, C, stats, gv_weight, gv_iters, trace, device_index, em=None):
    """What conversion_trajectory and conversion_trajectory_em share, from a validated dynamic map `v` and validated
    arguments: (rows, the ascent's objective or None, the refinement's mean log-likelihoods or None).  `em` is None or
    dict(iters, tol, trace); with None or iters = 0 the device work is conversion_trajectory's, launch for launch."""
    skip = 0 if v["level"] else 1
    span, dx, dy, M = v["span"], v["dx"], v["dy"], len(v["weights"])
    dxs, dys = dx // 2, dy // 2
    C = _cepstrum_rows(C, "C")
    if C.shape[1] != dxs + skip:
        raise ValueError("C must have %d columns for this conversion, got %d" % (dxs + skip, C.shape[1]))
    full, rows, out = _nonempty_rows(C, dys, skip)
    n = len(rows)
    if n == 0:
        return out, np.zeros((gv_iters + 1, dys)) if trace else None, np.zeros(1) if em and em["trace"] else None
    D = dynamic_rows(C, span, device_index=device_index)
    mu_c = v["means"] - v["zbar"]
    mix = _Mixture(_dynamic_columns(D[full], C.shape[1], skip), v["zbar"][:dx], M, device_index)
    gamma, _ = mix.estep(mu_c[:, :dx], v["Wx"], v["kx"])
    t, dev = mix.torch, mix.dev
    py = v["py"]
    r = t.empty((n, dy), dtype=t.float64, device=dev)
    pyA = t.as_tensor(np.ascontiguousarray(py[:, :, None] * v["A"]), device=dev)
    pyb = t.as_tensor(np.ascontiguousarray(py * (v["b"] + v["zbar"][dx:])), device=dev)
    mix.c.gmm_regress(mix.Z, gamma, pyA, pyb, n, dx, dy, M, r)
    py_d = t.as_tensor(py, device=dev)
    P = gamma @ py_d
    _, length = delta_runs(full)                       # the runs on the compacted rows: back to back
    start = np.concatenate(([0], np.cumsum(length)[:-1])).astype(np.int64)
    words = mix.c.mlpg_work_len(n, dys, span)
    _agree("the size of the trajectory solve's work buffer", words, mlpg_work_len(n, dys, span))
    Y = t.empty((n, dys), dtype=t.float64, device=dev)
    P, start_d, length_d = P.contiguous(), t.as_tensor(start, device=dev), t.as_tensor(length, device=dev)
    work = t.empty(words, dtype=t.float64, device=dev)
    mix.c.mlpg_solve(P, r, n, dys, span, start_d, length_d, len(start), work, Y)
    loglik = None
    if em and (em["iters"] or em["trace"]):            # X, pi = gamma, the scaled parameters, the runs and work stay put
        kc = 0.5 * np.log(py).sum(axis=1) - dys * math.log(2.0 * math.pi)
        A_d, bq_d, kc_d = (t.as_tensor(np.ascontiguousarray(a), device=dev) for a in (v["A"], v["b"] + v["zbar"][dx:], kc))
        refined = t.empty((n, M), dtype=t.float64, device=dev)
        ll = t.empty(n, dtype=t.float64, device=dev)
        score = em["trace"] or em["tol"] > 0           # the only read-back of the loop: n doubles per E-step
        means = []

        def estep():
            mix.c.mlpg_estep(mix.Z, gamma, A_d, bq_d, py_d, kc_d, Y, n, dx, dys, M, span, start_d, length_d, len(start),
                             refined, ll)
            if score:
                means.append(math.fsum(ll.cpu().numpy()) / n)
        stopped = False
        for _ in range(em["iters"]):
            estep()
            if em["tol"] > 0 and len(means) > 1 and means[-1] - means[-2] < em["tol"]:
                stopped = True                         # Y is the trajectory this E-step scored; P and r are the ones behind it
                break
            P = (refined @ py_d).contiguous()
            mix.c.gmm_regress(mix.Z, refined, pyA, pyb, n, dx, dy, M, r)
            mix.c.mlpg_solve(P, r, n, dys, span, start_d, length_d, len(start), work, Y)
        if em["trace"]:
            if not stopped:
                estep()                                # the last trajectory's score; P and r do not follow it
            loglik = np.array(means)
    objective = None
    if stats is not None:                              # P, r, the runs and y_ML stay where they are
        words = mix.c.gv_work_len(n, dys, span)
        _agree("the size of the global-variance ascent's work buffer", (words, mix.c.gv_chunk_rows(n)),
               (gv_work_len(n, dys, span), gv_chunk_rows(n)))
        if trace:
            objective = t.empty((gv_iters + 1, dys), dtype=t.float64, device=dev)
        mix.c.gv_ascend(P, r, n, dys, span, start_d, length_d, len(start), t.as_tensor(stats["gv_mean"], device=dev),
                        t.as_tensor(gv_weight * stats["gv_prec"], device=dev), gv_iters,
                        t.empty(words, dtype=t.float64, device=dev), Y, objective)
    out = _put_rows(out, full, skip, C, Y.cpu().numpy())
    return out, objective.cpu().numpy() if trace else None, loglik


# ---- pitch (host only)
def _f0_track(f0, voiced):
    f = _numeric_1d(f0, "f0")
    vo = np.asarray(voiced)
    if vo.shape != f.shape or vo.dtype.kind not in "biu":
        raise ValueError("voiced must be one flag per entry of f0")
    vo = vo.astype(bool)
    if not (np.all(np.isfinite(f[vo])) and np.all(f[vo] > 0)):
        raise ValueError("f0 must be finite and > 0 at the voiced instants")
    return f, vo


def f0_statistics(f0, voiced):
    """(mean, std) of ln f0 over the voiced instants (population std); ValueError without a voiced instant."""
    f, vo = _f0_track(f0, voiced)
    if not vo.any():
        raise ValueError("f0_statistics needs at least one voiced instant")
    lf = np.log(f[vo])
    return float(lf.mean()), float(lf.std())


def _stats(s, name):
    try:
        m, d = (float(x) for x in s)
    except (TypeError, ValueError):
        raise ValueError("%s must be (mean, std) of ln f0" % name) from None
    if not (np.isfinite(m) and np.isfinite(d) and d >= 0):
        raise ValueError("%s must be finite with std >= 0" % name)
    return m, d


def pitch_conversion_contour(f0, voiced, src_stats, tgt_stats):
    """The log-Gaussian normalisation of pitch: ln f0' = mean_t + (std_t / std_s) (ln f0 - mean_s) at the voiced
    instants (std_s = 0: the ratio is 1).  Returns the pitch_scale contour f0' / f0, float64[n], clipped to SCALE_RANGE,
    1 at the unvoiced instants.  Host only."""
    f, vo = _f0_track(f0, voiced)
    (ms, ds), (mt, dt) = _stats(src_stats, "src_stats"), _stats(tgt_stats, "tgt_stats")
    ratio = dt / ds if ds > 0 else 1.0
    out = np.ones(len(f))
    lf = np.log(f[vo])
    with np.errstate(over="ignore"):
        out[vo] = np.clip(np.exp(mt + ratio * (lf - ms) - lf), *SCALE_RANGE)
    return out
