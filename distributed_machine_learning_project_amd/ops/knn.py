"""Local (single-device) exact k-NN: the compute backend every parallel strategy calls.

GPU: libdmlp's ONE native pipeline (csrc/pipeline.hip), which the standalone knn_engine and the
engine.h drop-in run as well — no part of a call is orchestrated from Python:
  knn_gpu  (dmlp_knn_local)  rows already on the device (shards, ring shards, out-of-core chunks):
           per-query classes — single-term MFMA screen (k <= 64), 3-term LDS screen (k <= 256),
           exact fp64 (k > 256, A > 256) — a device-rendered bf16 image, exact re-rank (reference
           order, no FMA), per-query escalation of overflowed screens, fused vote + FNV checksum
  step     (dmlp_step)       one rank's whole Engine::KNN call from host rows: the host renders
           the screen's fp16 operands while the GPU screens (early start), the fp64 rows cross
           PCIe behind the screen as lossless int32, exact re-rank, vote, checksum, the report
           text rendered on the GPU into page-locked host memory, one host sync
  vote_curve_gpu (dmlp_vote_curve)  the vote of every prefix of the sorted lists in one launch
           (csrc/vote_curve.hip): the votes of all k <= kmax for one search, leave-one-out hit counts
  vote_scores_gpu (dmlp_vote_scores)  per-class vote counts and uniform / inverse-squared-distance
           scores of the lists in one launch (csrc/vote_scores.hip): predict_proba, weighted predict
  neighbor_means_gpu / neighbor_means_curve_gpu (dmlp_neighbor_means, dmlp_neighbor_means_curve)
           the uniform / inverse-squared-distance mean of the neighbours' float targets, for the
           whole list or for every prefix of it, in one launch (csrc/neighbor_means.hip):
           KNNRegressor's predict, predict_curve and leave-one-out curves
  radius_count_gpu / radius_gpu (dmlp_radius_count, dmlp_radius_fill, dmlp_radius_sort)
           every point within a squared radius instead of the k nearest (csrc/radius.hip): two
           passes over the exact tier's fp64 distance tile, count then fill, and a stable segmented
           sort; CSR, or padded lists the list kernels above read with k = count
  radius_components_gpu (dmlp_radius_components)  connected components of the graph "within one
           squared radius" (csrc/components.hip): the same tile over the lower triangle of the rows
           against themselves, its hits united in a lock-free union-find as they appear; with
           exact_nearest_gpu (dmlp_exact_topk at k = 1 on raw device rows) what models.DBSCAN runs
CPU: libdmlp's threaded brute force (or the KD-tree of bench.debug), vote_curve_cpu,
vote_scores_cpu, neighbor_means_cpu, neighbor_means_curve_cpu, radius_count_cpu, radius_cpu,
radius_components_cpu.
curve_sse (host, both devices)
turns a mean curve into squared errors.  The eight list-kernel wrappers check and normalise their
lists in one place per backend (_host_lists, _device_lists), their weights in _weight_mode and
their curve length in _check_kcap.

Exactness contract (common.cpp:57-79, engine.cpp:12-18): distances are the
reference's left-to-right fp64 sums without FMA; the MFMA screens only filter candidates, with a
rigorous error bound, so results are bit-identical to the fp64 oracle.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from .. import _lib

SCREEN_KMAX_A = 64      # single-term one-pass screen class
SCREEN_KMAX_B = 128     # 3-term cap-256 class
SCREEN_KMAX_C = 256     # 3-term cap-512 class: larger k take the exact path
SCREEN_MAX_KT = 8       # A <= 256 on the screens


def screen_kt(A: int) -> int:
    """32-attribute fragments per row of the screen images (dmlp.h dmlp_screen_kt): A <= 256
    rounds up to 1, 2, 4 or 8, the single-term screen's variants."""
    kt = max(1, (A + 31) // 32)
    return kt if kt > 8 else 1 << (kt - 1).bit_length()


def eps_rel(A: int) -> float:
    """Relative error bound of the 3-term bf16 screen (pipeline.hip passes the same value)."""
    return 2.0 * (3.0 * 2.0 ** -16 + (3 * A + 8) * 2.0 ** -24)


# ======================================================================= CPU backend
def knn_cpu(X: np.ndarray, Qx: np.ndarray, k: np.ndarray, kstride: int | None = None,
            nthreads: int = 0, method: str = "brute"):
    """Exact top-k on the host.  Returns (dist [Q,kstride] f64, ids [Q,kstride] i32)."""
    X = np.ascontiguousarray(X, np.float64)
    Qx = np.ascontiguousarray(Qx, np.float64)
    k = np.ascontiguousarray(k, np.int32)
    Q = Qx.shape[0]
    ks = max(1, int(k.max()) if Q else 1) if kstride is None else kstride
    d = np.full((Q, ks), np.inf, np.float64)
    i = np.full((Q, ks), -1, np.int32)
    L = _lib.lib()
    if method == "kdtree":
        rc = L.dmlp_kdtree_knn(X.ctypes.data, X.shape[0], X.shape[1], Qx.ctypes.data, Q,
                               k.ctypes.data, ks, d.ctypes.data, i.ctypes.data)
    else:
        rc = L.dmlp_cpu_knn(X.ctypes.data, X.shape[0], X.shape[1], Qx.ctypes.data, Q,
                            k.ctypes.data, ks, d.ctypes.data, i.ctypes.data, nthreads)
    _lib.check(rc, "cpu knn")
    return d, i


def finalize_cpu(ids: np.ndarray, k: np.ndarray, labels: np.ndarray):
    ids = np.ascontiguousarray(ids, np.int32)
    k = np.ascontiguousarray(k, np.int32)
    labels = np.ascontiguousarray(labels, np.int32)
    Q = len(k)
    lab = np.empty(Q, np.int32)
    cs = np.empty(Q, np.uint64)
    _lib.check(_lib.lib().dmlp_cpu_finalize(None, ids.ctypes.data, ids.shape[1] if Q else 0,
                                            k.ctypes.data, Q, labels.ctypes.data,
                                            lab.ctypes.data, cs.ctypes.data), "cpu finalize")
    return lab, cs


VOTE_CURVE_KMAX = 256   # dmlp_vote_curve_kmax(): slots of a list the curve kernels read
VOTE_WEIGHTS = {"uniform": 0, "inv_sqdist": 1}  # the mode of the score and mean kernels


def _host_lists(ids, k, skip, dist, extra_q=()):
    """The list arguments every host list kernel takes, as contiguous arrays: ids int32 [Q, kstride]
    with kstride >= 1; k, skip and each of extra_q int32 [Q] (None stays None); dist float64 shaped
    like ids.  Returns ((ids, k, skip, dist, *extra_q), (Q, kstride)), or ValueError."""
    ids = np.ascontiguousarray(ids, np.int32)
    if ids.ndim != 2 or ids.shape[1] < 1:
        raise ValueError("ids must be [Q, kstride] with kstride >= 1")
    Q = ids.shape[0]
    k = np.ascontiguousarray(k, np.int32)
    skip, *extra_q = (None if a is None else np.ascontiguousarray(a, np.int32)
                      for a in (skip, *extra_q))
    dist = None if dist is None else np.ascontiguousarray(dist, np.float64)
    if any(a is not None and a.shape != (Q,) for a in (k, skip, *extra_q)) or \
            (dist is not None and dist.shape != ids.shape):
        raise ValueError("k, skip and truth must be [Q] and dist shaped like ids")
    return (ids, k, skip, dist, *extra_q), ids.shape


def _weight_mode(weights, have_dist: bool) -> int:
    """The kernels' mode of a `weights` name, or ValueError."""
    if weights not in VOTE_WEIGHTS:
        raise ValueError(f"weights must be one of {sorted(VOTE_WEIGHTS)}, not {weights!r}")
    if VOTE_WEIGHTS[weights] == 1 and not have_dist:
        raise ValueError("weights='inv_sqdist' needs dist")
    return VOTE_WEIGHTS[weights]


def _check_kcap(kcap, name: str = "kcap") -> int:
    kcap = int(kcap)
    if not 1 <= kcap <= VOTE_CURVE_KMAX:
        raise ValueError(f"{name} must be in [1, {VOTE_CURVE_KMAX}]")
    return kcap


def _curve_weighted(weights, score: bool, have_dist: bool):
    """The mode of a weighted vote-curve call (validated by _weight_mode), or None for the defaults,
    which take the unweighted entry."""
    mode = _weight_mode(weights, have_dist)
    return mode if (mode or score) else None


def vote_curve_cpu(ids, k, labels, kcap: int, skip=None, truth=None, dist=None, hits=None, *,
                   weights: str = "uniform", score: bool = False, lists: bool = True):
    """The vote of every prefix of sorted lists (dmlp_cpu_vote_curve): ids [Q, kstride] int32, k
    [Q], labels [N]; skip [Q] drops one id per row (negative: none), entries with id < 0 are
    dropped too.  Returns (labels [Q, kcap] int32 — column j the vote over the first j + 1 kept
    entries, repeated past the last one, -1 for an empty row —, hits int64 [kcap] | None — with
    truth [Q]: rows whose column j equals truth, ADDED to `hits` when one is passed —, (dist, ids)
    [Q, kcap] | None — with dist: the kept entries, padded with (+inf, -1)).
    weights="inv_sqdist" (needs dist) or score=True take dmlp_cpu_vote_curve_weighted: column j is
    the class with the largest (score, count, label) over the first j + 1 kept entries, a class's
    score the sum in list order of 1 / d over its entries (d: the engine's SQUARED distances; a row
    whose first kept entry sits at d == 0 counts the entries at 0 as 1 and every other as 0);
    score=True appends the winners' scores, float64 [Q, kcap] (uniform: the counts), as a fourth
    element; lists=False leaves the third None although dist is given (a weighted caller that
    wants the votes only)."""
    mode = _curve_weighted(weights, score, dist is not None)
    (ids, k, skip, dist, truth), (Q, ks) = _host_lists(ids, k, skip, dist, (truth,))
    labels = np.ascontiguousarray(labels, np.int32)
    kcap = _check_kcap(kcap)
    lab = np.empty((Q, kcap), np.int32)
    lists = bool(lists) and dist is not None
    od = np.empty((Q, kcap), np.float64) if lists else None
    oi = np.empty((Q, kcap), np.int32) if lists else None
    if truth is not None:
        if hits is None:
            hits = np.zeros(kcap, np.int64)
        elif hits.dtype != np.int64 or hits.shape != (kcap,) or not hits.flags.c_contiguous:
            raise ValueError("hits must be a contiguous int64 [kcap] array")
    else:
        hits = None
    lists = (od, oi) if lists else None
    if mode is None:
        _lib.check(_lib.lib().dmlp_cpu_vote_curve(
            _np_ptr(dist), ids.ctypes.data, ks, k.ctypes.data, Q, _np_ptr(skip),
            labels.ctypes.data, kcap, lab.ctypes.data, _np_ptr(od), _np_ptr(oi), _np_ptr(truth),
            _np_ptr(hits)), "cpu vote curve")
        return lab, hits, lists
    sc = np.empty((Q, kcap), np.float64) if score else None
    _lib.check(_lib.lib().dmlp_cpu_vote_curve_weighted(
        _np_ptr(dist), ids.ctypes.data, ks, k.ctypes.data, Q, _np_ptr(skip), labels.ctypes.data,
        mode, kcap, lab.ctypes.data, _np_ptr(sc), _np_ptr(od), _np_ptr(oi), _np_ptr(truth),
        _np_ptr(hits)), "cpu weighted vote curve")
    return (lab, hits, lists, sc) if score else (lab, hits, lists)


VOTE_SCORES_CMAX = 4096  # dmlp_vote_scores_cmax(): classes a score launch takes


def _score_mode(label_lo, nclass, weights, have_dist: bool):
    """(label_lo, nclass, mode) of a class-score call, or ValueError for what the C entry rejects."""
    mode = _weight_mode(weights, have_dist)
    nclass = int(nclass)
    if not 1 <= nclass <= VOTE_SCORES_CMAX:
        raise ValueError(f"nclass must be in [1, {VOTE_SCORES_CMAX}]")
    label_lo = int(label_lo)
    if not -(1 << 31) <= label_lo < (1 << 31):
        raise ValueError("label_lo must be an int32")
    return label_lo, nclass, mode


def vote_scores_cpu(ids, k, labels, label_lo: int, nclass: int, weights: str = "uniform",
                    dist=None, skip=None):
    """Per-class votes of neighbour lists (dmlp_cpu_vote_scores): ids [Q, kstride] int32, k [Q],
    labels [N]; the first min(k_q, kstride) slots of a row are read, whatever their number; entries
    with id < 0, with id == skip_q (skip [Q], negative: none) or with a label outside [label_lo,
    label_lo + nclass) are dropped.  Returns (count [Q, nclass] int32, score [Q, nclass] float64,
    label [Q] int32): weights="uniform" scores a class by its count; "inv_sqdist" by the sum, in
    list order, of 1 / d over its entries (d: dist, shaped like ids, the engine's SQUARED distances;
    a row with an entry at d == 0 counts those entries 1 and every other 0).  label is the class
    with the largest (score, count, label), -1 for a row that keeps nothing."""
    (ids, k, skip, dist), (Q, ks) = _host_lists(ids, k, skip, dist)
    label_lo, nclass, mode = _score_mode(label_lo, nclass, weights, dist is not None)
    labels = np.ascontiguousarray(labels, np.int32)
    count = np.empty((Q, nclass), np.int32)
    score = np.empty((Q, nclass), np.float64)
    lab = np.empty(Q, np.int32)
    _lib.check(_lib.lib().dmlp_cpu_vote_scores(
        _np_ptr(dist), ids.ctypes.data, ks, k.ctypes.data, Q, _np_ptr(skip), labels.ctypes.data,
        label_lo, nclass, mode, count.ctypes.data, score.ctypes.data, lab.ctypes.data),
        "cpu vote scores")
    return count, score, lab


def class_proba(score, count):
    """Class probabilities [Q, C] float64 of the (score, count) a class-score call returned, as host
    arrays — one function for both devices, so their probabilities agree bit for bit.  Per row:
    score / total (total: the sum over classes); total == 0 (every neighbour at +inf): count / m
    (m: the kept entries); no kept entry: zeros; a score at +inf: 1 / n_inf on those classes and 0
    elsewhere.  `count` may be a callable returning the array: it is called only when a row's
    scores sum to 0.  (Finite scores whose sum overflows are scaled by 2^-13 first, enough
    for 4096 classes, rather than divided by +inf.)"""
    score = np.ascontiguousarray(score, np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        total = score.sum(axis=1, keepdims=True)
        inf = np.isinf(score)
        has_inf = inf.any(axis=1, keepdims=True)
        over = np.isinf(total) & ~has_inf
        if over.any():
            small = score * 2.0 ** -13
            score = np.where(over, small, score)
            total = np.where(over, small.sum(axis=1, keepdims=True), total)
        p = score / total
        p = np.where(has_inf, inf / inf.sum(axis=1, keepdims=True), p)
        nothing = (total == 0).ravel()
        if nothing.any():
            cnt = np.asarray(count() if callable(count) else count)[nothing].astype(np.float64)
            m = cnt.sum(axis=1, keepdims=True)
            p[nothing] = np.where(m > 0, cnt / np.where(m > 0, m, 1.0), 0.0)
    return p


NEIGHBOR_MEANS_TMAX = 256  # dmlp_neighbor_means_tmax(): target columns a mean launch takes


def _means_args(T, weights, have_dist: bool, kcap=None):
    """(T, mode, kcap) of a neighbour-mean call, or ValueError for what the C entry rejects."""
    mode = _weight_mode(weights, have_dist)
    if not 1 <= T <= NEIGHBOR_MEANS_TMAX:
        raise ValueError(f"targets must have between 1 and {NEIGHBOR_MEANS_TMAX} columns")
    return int(T), mode, None if kcap is None else _check_kcap(kcap)


def _means_cpu_args(ids, k, targets, weights, dist, skip, kcap=None):
    (ids, k, skip, dist), _ = _host_lists(ids, k, skip, dist)
    targets = np.ascontiguousarray(targets, np.float64)
    if targets.ndim != 2:
        raise ValueError("targets must be [N, T]")
    T, mode, kcap = _means_args(targets.shape[1], weights, dist is not None, kcap)
    return ids, k, targets, dist, skip, T, mode, kcap


def neighbor_means_cpu(ids, k, targets, weights: str = "uniform", dist=None, skip=None):
    """The mean of the neighbours' targets (dmlp_cpu_neighbor_means): ids [Q, kstride] int32, k
    [Q], targets [N, T] float64, finite; the first min(k_q, kstride) slots of a row are read,
    whatever their number; entries with id < 0 or id == skip_q (skip [Q], negative: none) are
    dropped.  Returns (mean [Q, T] float64, wsum [Q] float64, count [Q] int32): weights="uniform"
    is the plain mean; "inv_sqdist" weighs an entry by d_ref / d (dist, shaped like ids, the
    engine's SQUARED distances; d_ref the first kept entry's), which is the mean under 1 / d
    weights: a row whose first kept entry sits at d == 0 averages its entries at d == 0 only.
    Sums run in list order, left to right, without FMA; a row that keeps nothing is NaN with wsum
    0 and count 0."""
    ids, k, targets, dist, skip, T, mode, _ = _means_cpu_args(ids, k, targets, weights, dist, skip)
    Q, ks = ids.shape
    mean = np.empty((Q, T), np.float64)
    wsum = np.empty(Q, np.float64)
    count = np.empty(Q, np.int32)
    _lib.check(_lib.lib().dmlp_cpu_neighbor_means(
        _np_ptr(dist), ids.ctypes.data, ks, k.ctypes.data, Q, _np_ptr(skip), targets.ctypes.data,
        T, mode, mean.ctypes.data, wsum.ctypes.data, count.ctypes.data), "cpu neighbor means")
    return mean, wsum, count


def neighbor_means_curve_cpu(ids, k, targets, kcap: int, weights: str = "uniform", dist=None,
                             skip=None):
    """The mean over every prefix of the lists (dmlp_cpu_neighbor_means_curve): float64 [Q, kcap,
    T], column j the mean over the first j + 1 kept entries of the first min(k_q, kstride, 256)
    slots — neighbor_means_cpu at that length, bit for bit —, repeated past the last kept entry,
    NaN for a row that keeps nothing.  Arguments as for neighbor_means_cpu."""
    ids, k, targets, dist, skip, T, mode, kcap = _means_cpu_args(ids, k, targets, weights, dist,
                                                                 skip, kcap)
    Q, ks = ids.shape
    mean = np.empty((Q, kcap, T), np.float64)
    _lib.check(_lib.lib().dmlp_cpu_neighbor_means_curve(
        _np_ptr(dist), ids.ctypes.data, ks, k.ctypes.data, Q, _np_ptr(skip), targets.ctypes.data,
        T, mode, kcap, mean.ctypes.data), "cpu neighbor means curve")
    return mean


def curve_sse(mean, truth):
    """float64 [kcap, T]: the squared error of every column of a mean curve, summed over the rows
    — ((mean - truth[:, None, :]) ** 2).sum(axis=0) for mean [R, kcap, T] and truth [R, T], as host
    arrays.  One function for both devices, so their leave-one-out errors agree bit for bit."""
    mean = np.ascontiguousarray(mean, np.float64)
    truth = np.ascontiguousarray(truth, np.float64)
    if mean.ndim != 3 or truth.shape != (mean.shape[0], mean.shape[2]):
        raise ValueError("mean must be [R, kcap, T] and truth [R, T]")
    with np.errstate(over="ignore", invalid="ignore"):
        return ((mean - truth[:, None, :]) ** 2).sum(axis=0)


def merge_cpu(lists_d: np.ndarray, lists_i: np.ndarray, k: np.ndarray, kout: int | None = None):
    """lists_*: [L, Q, kin] sorted per-shard top-k lists -> merged [Q, kout]."""
    Ld = np.ascontiguousarray(lists_d, np.float64)
    Li = np.ascontiguousarray(lists_i, np.int32)
    k = np.ascontiguousarray(k, np.int32)
    L, Q, kin = Ld.shape
    kout = kout or max(1, int(k.max()) if Q else 1)
    d = np.full((Q, kout), np.inf, np.float64)
    i = np.full((Q, kout), -1, np.int32)
    _lib.check(_lib.lib().dmlp_cpu_merge(Ld.ctypes.data, Li.ctypes.data, L, Q * kin, kin,
                                         k.ctypes.data, Q, d.ctypes.data, i.ctypes.data, kout),
               "cpu merge")
    return d, i


RADIUS_SPAN_MAX = (1 << 31) - 1  # slots one fill + sort call addresses (32-bit segment offsets)


def _radius_layout(count_max: int, total, Q: int, stride):
    """The slots a radius fill addresses: `total` (CSR) or (Q - 1) stride + the largest count
    (padded lists at stride `stride`, which must hold every count), or ValueError."""
    if stride is None:
        span = int(total)
    else:
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be >= 1")
        if count_max > stride:
            raise ValueError(f"a query has {count_max} neighbours: more than stride {stride}")
        span = (Q - 1) * stride + count_max if Q else 0
    if span > RADIUS_SPAN_MAX:
        raise ValueError(f"{span} slots in one radius call: at most {RADIUS_SPAN_MAX}, batch the "
                         "queries")
    return span


def _radius_host_args(X, Qx, r2):
    X = np.ascontiguousarray(X, np.float64)
    Qx = np.ascontiguousarray(Qx, np.float64)
    if X.ndim != 2 or Qx.ndim != 2 or X.shape[1] != Qx.shape[1] or X.shape[1] < 1:
        raise ValueError("X must be [N, A] and Qx [Q, A] with A >= 1")
    r2 = np.asarray(r2, np.float64)
    if r2.ndim == 0:
        r2 = np.full(Qx.shape[0], float(r2), np.float64)
    r2 = np.ascontiguousarray(r2)
    if r2.shape != (Qx.shape[0],):
        raise ValueError("r2 must be a scalar or [Q]")
    return X, Qx, r2


def radius_count_cpu(X, Qx, r2, nthreads: int = 0):
    """int32 [Q]: the points of X [N, A] within the SQUARED radius r2 (a scalar or [Q] float64) of
    each query row of Qx [Q, A], the boundary included (dmlp_cpu_radius_count): dist(q, x) <= r2_q
    in the engine's distance.  A negative or NaN r2 counts nothing, +inf every point."""
    X, Qx, r2 = _radius_host_args(X, Qx, r2)
    Q = Qx.shape[0]
    count = np.zeros(Q, np.int32)
    _lib.check(_lib.lib().dmlp_cpu_radius_count(
        X.ctypes.data if X.size else None, X.shape[0], X.shape[1], Qx.ctypes.data, Q,
        r2.ctypes.data, count.ctypes.data, nthreads), "cpu radius count")
    return count


def radius_cpu(X, Qx, r2, sort: bool = True, stride=None, count=None, nthreads: int = 0):
    """Every point within the squared radius r2 of each query (dmlp_cpu_radius_fill), ordered by
    (dist asc, id desc) — the first count_q entries of the query's exact k-NN list — or, with
    sort=False, by descending id.  stride=None: CSR (indptr int64 [Q + 1], dist float64 [total],
    ids int32 [total]).  stride=s: padded lists (dist [Q, s], ids [Q, s], count int32 [Q]), slots
    past count_q holding (+inf, -1): what vote_scores_cpu and neighbor_means_cpu read with k =
    count; a count above s is a ValueError.  count: radius_count_cpu's result for the same
    arguments, when the caller has it."""
    X, Qx, r2 = _radius_host_args(X, Qx, r2)
    Q = Qx.shape[0]
    if count is None:
        count = radius_count_cpu(X, Qx, r2, nthreads)
    count = np.ascontiguousarray(count, np.int32)
    if count.shape != (Q,):
        raise ValueError("count must be [Q]")
    indptr = np.zeros(Q + 1, np.int64)
    np.cumsum(count, out=indptr[1:])
    _radius_layout(int(count.max()) if Q else 0, indptr[Q], Q, stride)
    if stride is None:
        off = indptr[:Q]
        d = np.empty(int(indptr[Q]), np.float64)
        i = np.empty(int(indptr[Q]), np.int32)
    else:
        off = np.arange(Q, dtype=np.int64) * int(stride)
        d = np.full((Q, int(stride)), np.inf, np.float64)
        i = np.full((Q, int(stride)), -1, np.int32)
    if d.size:
        _lib.check(_lib.lib().dmlp_cpu_radius_fill(
            X.ctypes.data if X.size else None, X.shape[0], X.shape[1], Qx.ctypes.data, Q,
            r2.ctypes.data, count.ctypes.data, np.ascontiguousarray(off).ctypes.data,
            d.ctypes.data, i.ctypes.data, 1 if sort else 0, nthreads), "cpu radius fill")
    return (indptr, d, i) if stride is None else (d, i, count)


def _components_r2(r2) -> float:
    try:
        return float(r2)
    except (TypeError, ValueError):
        raise ValueError("r2 must be one float, the SQUARED radius") from None


def radius_components_cpu(X, r2, nthreads: int = 0):
    """int32 [N]: comp[i] = the smallest row id in the connected component of row i of X [N, A]
    under the edges dist(x_i, x_j) <= r2 (dmlp_cpu_radius_components) — r2 ONE squared radius, the
    boundary included; a negative or NaN r2 links nothing, +inf every pair."""
    X = np.ascontiguousarray(X, np.float64)
    if X.ndim != 2 or X.shape[1] < 1:
        raise ValueError("X must be [N, A] with A >= 1")
    comp = np.empty(X.shape[0], np.int32)
    if X.shape[0]:
        _lib.check(_lib.lib().dmlp_cpu_radius_components(
            X.ctypes.data, X.shape[0], X.shape[1], _components_r2(r2), comp.ctypes.data, nthreads),
            "cpu radius components")
    return comp


# ======================================================================= GPU backend
def _torch():
    import torch
    return torch


_RAW_STREAM = []


def _stream():
    """The current stream's raw handle, without building a torch Stream object."""
    torch = _torch()
    if not _RAW_STREAM:
        _RAW_STREAM.append(getattr(torch._C, "_cuda_getCurrentRawStream", None))
    f = _RAW_STREAM[0]
    if f is not None:
        return f(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("native kernels need contiguous tensors")
    return t.data_ptr()


def _np_ptr(a):
    return None if a is None else a.ctypes.data


# ---------------------------------------------------------------- pipeline switches + stats
@contextlib.contextmanager
def pipeline_options(**kw):
    """Tuning / A-B switches of the native pipeline for the duration of a block (pipeline.hip
    Tuning): num_cus (CUs the slice choice fills), screen (first screen of the k <= 32 class on
    the device image: 0 single-term, 1 3-term streaming, 2 3-term LDS; != 0 also turns the host
    operands off), x1k (two-pass single-term screen for k in (32, 256]), host_ops."""
    L = _lib.lib()
    names = {"screen": {"x1": 0, "stream": 1, "lds": 2}}
    old = {}
    try:
        for key, v in kw.items():
            v = names.get(key, {}).get(v, v)
            prev = L.dmlp_pipeline_set(key.encode(), int(v))
            if prev < 0:
                raise KeyError(key)
            old[key] = prev
        yield
    finally:
        for key, v in old.items():
            L.dmlp_pipeline_set(key.encode(), v)


def pipeline_stats():
    """What the last native call did: {"n_exact", "n_escalated", "path", "early", "n_exact_f64",
    "n_exact_f64_redo", "device_render", "report_direct"} (exact-path queries on the fp64 MFMA
    screen, and those of them that overflowed to the fused VALU kernel; whether the GPU rendered
    the screen operands; whether the report text went straight into the caller's page-locked
    buffer)."""
    out = (C.c_int64 * 8)()
    _lib.lib().dmlp_pipeline_stats(out)
    return {"n_exact": out[0], "n_escalated": out[1], "path": out[2], "early": out[3],
            "n_exact_f64": out[4], "n_exact_f64_redo": out[5], "device_render": out[6],
            "report_direct": out[7]}


# ---------------------------------------------------------------- rows on the device
@dataclass
class DeviceDataset:
    """A dataset resident on one GPU (fp64 rows + labels); the native pipeline renders its
    screen image inside each call (timed, like the reference's pack/scatter)."""
    X: "object"            # torch f64 [N, A] (cuda)
    labels: "object"       # torch i32 [N] or None
    label_lo: int
    label_hi: int

    @property
    def N(self):
        return self.X.shape[0]

    @property
    def A(self):
        return self.X.shape[1]

    @property
    def KT(self):
        return screen_kt(self.A)


def prepare_dataset(X, labels=None, label_range=None) -> DeviceDataset:
    torch = _torch()
    X = X.contiguous()
    assert X.is_cuda and X.dtype == torch.float64 and X.dim() == 2
    N = X.shape[0]
    if labels is not None:
        labels = labels.to(device=X.device, dtype=torch.int32).contiguous()
        if label_range is None:
            lo = int(labels.min().item()) if N else 0
            hi = int(labels.max().item()) + 1 if N else 1
        else:
            lo, hi = label_range
    else:
        lo, hi = 0, 1
    return DeviceDataset(X, labels, lo, hi)


@dataclass
class DeviceResult:
    dist: "object"     # torch f64 [Q, kstride]
    ids: "object"      # torch i32 [Q, kstride]
    label: "object"    # torch i32 [Q] or None
    checksum: "object"  # torch i64 [Q] (uint64 bits) or None
    k: np.ndarray
    n_fallback: int = 0    # queries answered by the exact fp64 path
    n_escalated: int = 0   # single-term screen overflows re-screened with a 3-term screen


def knn_gpu(ds: DeviceDataset, Qx, k_host: np.ndarray, finalize: bool = True,
            exact: bool = False, kstride: int | None = None) -> DeviceResult:
    """Exact top-k of every query row of Qx (torch f64 cuda [Q, A]) against ds
    (dmlp_knn_local).  k_host: numpy int32 [Q]; returns once the results are complete."""
    torch = _torch()
    Qx = Qx.contiguous()
    Q = Qx.shape[0]
    k_host = np.ascontiguousarray(k_host, np.int32)
    ks = max(1, int(k_host.max()) if Q else 1) if kstride is None else kstride
    dev = Qx.device
    od = torch.empty((Q, ks), dtype=torch.float64, device=dev)
    oi = torch.empty((Q, ks), dtype=torch.int32, device=dev)
    fin = finalize and ds.labels is not None
    lab = torch.empty(Q, dtype=torch.int32, device=dev) if fin else None
    cs = torch.empty(Q, dtype=torch.int64, device=dev) if fin else None
    _lib.check(_lib.lib().dmlp_knn_local(
        _p(ds.X), ds.N, ds.A, _p(Qx), Q, k_host.ctypes.data, ks, _p(od), _p(oi),
        _p(ds.labels) if fin else None, ds.label_lo, ds.label_hi, _p(lab), _p(cs),
        1 if exact else 0, _stream()), "knn_local")
    st = pipeline_stats()
    return DeviceResult(od, oi, lab, cs, k_host, int(st["n_exact"]), int(st["n_escalated"]))


# ---------------------------------------------------------------- one rank's call from host rows
class StepArgs(C.Structure):
    """dmlp.h dmlp_step_args."""
    _fields_ = [("X", C.c_void_p), ("Xr", C.c_void_p), ("N", C.c_int64), ("A", C.c_int),
                ("labels", C.c_void_p), ("label_lo", C.c_int), ("label_hi", C.c_int),
                ("Qx", C.c_void_p), ("Qr", C.c_void_p), ("k", C.c_void_p), ("Q", C.c_int64),
                ("kmin", C.c_int), ("kmax", C.c_int), ("qid_base", C.c_int64),
                ("exact", C.c_int), ("out_lab", C.c_void_p), ("out_cs", C.c_void_p),
                ("out_d", C.c_void_p), ("out_i", C.c_void_p), ("kstride", C.c_int),
                ("report_mode", C.c_int), ("report_dst", C.c_void_p), ("report_cap", C.c_int64),
                ("stream", C.c_void_p), ("plane", C.c_void_p), ("report_len", C.c_int64),
                ("path", C.c_int),
                ("early", C.c_int), ("n_escalated", C.c_int), ("early_waits", C.c_int),
                ("early_grows", C.c_int), ("early_timeouts", C.c_int),
                ("host_ms", C.c_float), ("X32d", C.c_void_p)]


class Plane(C.Structure):
    """dmlp.h dmlp_plane: the node render plane (csrc/plane.cpp)."""
    _fields_ = [("base", C.c_void_p), ("bytes", C.c_int64), ("rank", C.c_int),
                ("renderers", C.c_int), ("with_f64", C.c_int), ("pad_", C.c_int),
                ("gen", C.c_int64), ("wait_s", C.c_double)]


@dataclass
class StepResult:
    label: "object"        # torch i32 [Q] (device)
    checksum: "object"     # torch i64 [Q] (device, uint64 bits)
    dist: "object"         # torch f64 [Q, kstride] or None (lists=False)
    ids: "object"
    report_len: int        # report bytes (in dst, or on the device for step_emit)
    path: int              # 0 host-rendered screen operands, 2 device image
    early: int             # the screen started before the dataset image landed
    n_escalated: int
    n_fallback: int
    early_waits: int = 0
    early_grows: int = 0
    early_timeouts: int = 0


# calls the native step served and its early-start counters (bench.py reports them for the timed
# region; tests check that the early start ran)
STEP_STATS = {"calls": 0, "early": 0, "early_waits": 0, "early_grows": 0, "early_timeouts": 0,
              "escalated": 0, "device_path": 0, "host_ms": 0.0}
_IO = {"h2d": 0, "d2h": 0}  # host <-> device bytes the steps issued (bench.py diagnostics)


def step_stats(reset: bool = False):
    out = dict(STEP_STATS)
    if reset:
        for key in STEP_STATS:
            STEP_STATS[key] = 0
    return out


def step(X_host, labels_host, label_range, Q_host, k_host, *, k_range=None, qid_base=0,
         exact=False, report=None, lists=False, kstride=None, plane=None,
         x32=None) -> StepResult:
    """One rank's whole Engine::KNN call from host arrays (dmlp_step): X_host [N, A] /
    Q_host [Q, A] fp64, labels_host [N] int32 (page-locked or registered memory for real
    overlap; a node-shared segment is), k_host [Q] int32.
      report: None — no text; a page-locked uint8 numpy array of >= dmlp_format_bound(Q) bytes —
              the "Query <id> checksum: <u64>" lines land there (ids from qid_base); "device" —
              kept on the GPU for step_emit (the multi-rank egress).
      lists:  also return the sorted (dist, id) lists [Q, kstride] (the DEBUG listing).
      k_range: (a lower bound of min k, an upper bound of max k) when known, else scanned.
      plane:  a Plane (node render plane): the dataset's image and rows are rendered once per
              node, slice by slice, by the plane's renderers into a node-shared segment.
      x32:    the dataset's rows already on this GPU as lossless int32 [N * A] (a torch tensor:
              the xGMI replica, parallel/strategies.py): no dataset rows cross PCIe.
    Returns once everything is complete (one host sync in the common case)."""
    torch = _torch()
    L = _lib.lib()
    X_host = np.ascontiguousarray(X_host, np.float64)
    Q_host = np.ascontiguousarray(Q_host, np.float64)
    k_host = np.ascontiguousarray(k_host, np.int32)
    labels_host = None if labels_host is None else np.ascontiguousarray(labels_host, np.int32)
    N, A = X_host.shape
    Q = Q_host.shape[0]
    if Q and k_range is None and lists and not kstride:
        k_range = _lib.i32_range(k_host)  # (the lists' stride)
    if k_range is None:  # the native step scans k on its render pool
        kmin, kmax = (1, 0) if Q else (1, 1)
    else:
        kmin, kmax = (int(k_range[0]), int(k_range[1])) if Q else (1, 1)
    ks = kstride or (max(1, kmax) if kmax >= kmin else 0)
    dev = torch.device("cuda", torch.cuda.current_device())
    lab = torch.empty(max(Q, 1), dtype=torch.int32, device=dev)[:Q]
    cs = torch.empty(max(Q, 1), dtype=torch.int64, device=dev)[:Q]
    od = oi = None
    if lists:
        od = torch.empty((Q, ks), dtype=torch.float64, device=dev)
        oi = torch.empty((Q, ks), dtype=torch.int32, device=dev)
    a = StepArgs()
    a.X, a.N, a.A = _np_ptr(X_host), N, A
    a.labels = _np_ptr(labels_host)
    # (label_range None: the native step scans the labels on its render pool)
    a.label_lo, a.label_hi = (int(label_range[0]), int(label_range[1])) if label_range else (0, 0)
    a.Qx, a.k, a.Q = _np_ptr(Q_host), _np_ptr(k_host), Q
    a.kmin, a.kmax = kmin, kmax
    a.qid_base = int(qid_base)
    a.exact = 1 if exact else 0
    a.out_lab, a.out_cs = _p(lab), _p(cs)
    a.out_d, a.out_i = _p(od), _p(oi)
    a.kstride = ks
    if report is None or labels_host is None:
        a.report_mode = 0
    elif isinstance(report, str):
        if report != "device":
            raise ValueError(report)
        a.report_mode = 2
    else:
        a.report_mode = 1
        a.report_dst, a.report_cap = report.ctypes.data, report.nbytes
    a.stream = _stream()
    a.plane = C.cast(C.pointer(plane), C.c_void_p) if plane is not None else None
    a.X32d = x32.data_ptr() if x32 is not None else None
    _lib.check(L.dmlp_step(C.byref(a)), "dmlp_step")
    st = pipeline_stats()
    STEP_STATS["calls"] += 1
    STEP_STATS["early"] += a.early
    STEP_STATS["early_waits"] += a.early_waits
    STEP_STATS["early_grows"] += a.early_grows
    STEP_STATS["early_timeouts"] += a.early_timeouts
    STEP_STATS["host_ms"] += a.host_ms
    STEP_STATS["escalated"] += a.n_escalated
    STEP_STATS["device_path"] += 1 if a.path == 2 else 0
    kt = screen_kt(A)
    _IO["h2d"] += ((N + 63) // 64 * 64 * (kt * 64 + 4) + Q * (kt * 64 + 4) if a.path == 0 else 0)
    _IO["h2d"] += (Q if x32 is not None else N + Q) * A * 4 + N * 4  # (lossless int32 rows)
    if a.report_mode == 1:  # (written straight across PCIe: the text; else the staged bound)
        _IO["d2h"] += int(a.report_len) if st["report_direct"] else L.dmlp_format_bound(Q)
    if _EVENTS[0]:
        _read_timeline()
    return StepResult(lab, cs, od, oi, int(a.report_len), a.path, a.early, a.n_escalated,
                      int(st["n_exact"]), a.early_waits, a.early_grows, a.early_timeouts)


def step_emit(dst, nbytes: int):
    """The last step's report bytes (report="device") -> dst (page-locked / registered uint8
    numpy view of >= nbytes), synchronously."""
    if nbytes:
        _lib.check(_lib.lib().dmlp_step_emit(dst.ctypes.data, int(nbytes), _stream()), "step_emit")
        _IO["d2h"] += int(nbytes)


def knn_gpu_pipelined(X_host, labels_host, label_range, Q_host, k_host, kstride=None,
                      finalize=True, exact=False, k_range=None):
    """step() with the sorted lists out (the DEBUG listing, tests): returns (info, dist, ids,
    label, checksum, n_fallback); info.hl is 1 when the host rendered the screen operands, 2 for
    the device image path."""
    r = step(X_host, labels_host if finalize else None, label_range, Q_host, k_host,
             k_range=k_range, exact=exact, lists=True, kstride=kstride)

    @dataclass
    class _Info:
        hl: int
        early: int
        n_escalated: int
    return (_Info(1 if r.path == 0 else 2, r.early, r.n_escalated), r.dist, r.ids,
            r.label if finalize else None, r.checksum if finalize else None, r.n_fallback)


def io_bytes(reset: bool = False):
    out = dict(_IO)
    if reset:
        _IO["h2d"] = _IO["d2h"] = 0
    return out


# ---------------------------------------------------------------- step timeline (hipEvents)
_EVENTS = [os.environ.get("DMLP_PIPE_EVENTS") == "1"]
_LAST_TIMELINE = []


def set_pipe_events(on: bool):
    _EVENTS[0] = bool(on)
    _lib.lib().dmlp_step_events(1 if on else 0)


def _read_timeline():
    global _LAST_TIMELINE
    ms = (C.c_double * 16)()
    names = (C.c_char_p * 16)()
    m = _lib.lib().dmlp_step_timeline(ms, names, 16)
    _LAST_TIMELINE = [(names[i].decode(), round(ms[i], 4)) for i in range(m)]


def pipe_timeline():
    return list(_LAST_TIMELINE)


# ---------------------------------------------------------------- out-of-core, merge, finalize
def _side_stream(name, _cache={}):
    torch = _torch()
    key = (name, torch.cuda.current_device())
    st = _cache.get(key)
    if st is None:
        st = _cache[key] = torch.cuda.Stream()
    return st


def knn_gpu_streamed(X_host, labels_host, label_range, Qx, k_host, chunk_rows: int,
                     kstride=None, exact: bool = False):
    """Out-of-core exact k-NN ("stream from host memory beyond HBM"): the dataset
    stays in (page-locked) host memory and crosses PCIe in chunks of chunk_rows rows, double
    buffered on a copy stream so chunk c+1 is in flight while chunk c is screened; each chunk's
    top-k lists (global ids) are merged into the running lists by the K-way merge kernel, and
    the vote / checksum run once at the end.  Device memory: 2 chunks + queries + labels.
    Returns (dist, ids, label, checksum) on the current device."""
    torch = _torch()
    dev = Qx.device
    main = torch.cuda.current_stream()
    copy = _side_stream("h2d")
    N, A = X_host.shape
    Q = Qx.shape[0]
    k_host = np.ascontiguousarray(k_host, np.int32)
    ks = max(1, int(k_host.max()) if Q else 1) if kstride is None else kstride
    chunk_rows = max(1, min(int(chunk_rows), N))
    nchunks = (N + chunk_rows - 1) // chunk_rows
    bufs = [torch.empty((chunk_rows, A), dtype=torch.float64, device=dev) for _ in range(2)]
    ready = [torch.cuda.Event() for _ in range(2)]
    freed = [None, None]
    labels = None
    copy.wait_stream(main)
    with torch.cuda.stream(copy):
        if labels_host is not None:
            labels = torch.from_numpy(np.ascontiguousarray(labels_host)).to(dev, non_blocking=True)

    def issue(c):
        b = c % 2
        a0, a1 = c * chunk_rows, min(N, (c + 1) * chunk_rows)
        if freed[b] is not None:
            copy.wait_event(freed[b])  # chunk c-2's screen is done with this buffer
        with torch.cuda.stream(copy):
            bufs[b][: a1 - a0].copy_(torch.from_numpy(np.ascontiguousarray(X_host[a0:a1])),
                                     non_blocking=True)
            ready[b].record(copy)
    issue(0)
    dr = ir = None
    kd = torch.from_numpy(k_host).to(dev)
    for c in range(nchunks):
        b = c % 2
        a0, a1 = c * chunk_rows, min(N, (c + 1) * chunk_rows)
        if c + 1 < nchunks:
            issue(c + 1)
        main.wait_event(ready[b])
        ds = prepare_dataset(bufs[b][: a1 - a0])
        r = knn_gpu(ds, Qx, k_host, finalize=False, exact=exact, kstride=ks)
        d, i = r.dist, torch.where(r.ids >= 0, r.ids + a0, r.ids)
        if dr is None:
            dr, ir = d, i
        else:
            dr, ir = merge_gpu(torch.stack([dr, d]), torch.stack([ir, i]), kd, ks)
        freed[b] = main.record_event()
    main.wait_stream(copy)
    lab = cs = None
    if labels is not None:
        lab, cs = finalize_gpu(labels, label_range, dr, ir, kd)
    return dr, ir, lab, cs


def merge_gpu(lists_d, lists_i, k_dev, kout: int):
    """lists_*: torch [L, Q, kin] sorted lists on one GPU -> merged [Q, kout] (K4)."""
    torch = _torch()
    Ld = lists_d.contiguous()
    Li = lists_i.contiguous()
    Lc, Q, kin = Ld.shape
    # dmlp_merge writes every slot of [0, kout), padding included: no fill pass
    out_d = torch.empty((Q, kout), dtype=torch.float64, device=Ld.device)
    out_i = torch.empty((Q, kout), dtype=torch.int32, device=Ld.device)
    _lib.check(_lib.lib().dmlp_merge(_p(Ld), _p(Li), Lc, Q * kin, kin, _p(k_dev), Q, _p(out_d),
                                     _p(out_i), kout, _stream()), "merge")
    return out_d, out_i


def finalize_gpu(ds_labels, label_range, dist, ids, k_dev):
    torch = _torch()
    Q, ks = ids.shape
    lab = torch.empty(Q, dtype=torch.int32, device=ids.device)
    cs = torch.empty(Q, dtype=torch.int64, device=ids.device)
    _lib.check(_lib.lib().dmlp_finalize(_p(dist), _p(ids), ks, _p(k_dev), None, Q, _p(ds_labels),
                                        label_range[0], label_range[1], _p(lab), _p(cs),
                                        _stream()), "finalize")
    return lab, cs


def _like_ids(t, ids):
    """t as a contiguous tensor of ids' dtype (int32) on ids' device; itself when it is one."""
    return None if t is None else t.to(ids).contiguous()


def _device_lists(ids, k, skip, dist, extra_q=()):
    """_host_lists for torch tensors on one GPU: ids must be an int32 tensor already, its device is
    the lists' device; k (a host array is copied over once), skip and each of extra_q end up int32
    [Q] there; dist must be float64, shaped like ids, on that device.  No work is issued for
    arguments that conform.  Returns ((ids, k, skip, dist, *extra_q), (Q, kstride)), or ValueError.
    (Every wrapper call passes through here: plain loops, no generators.)"""
    torch = _torch()
    if ids.dim() != 2 or ids.dtype != torch.int32 or ids.shape[1] < 1:
        raise ValueError("ids must be an int32 [Q, kstride] tensor with kstride >= 1")
    Q, ks = ids.shape
    if not torch.is_tensor(k):
        k = torch.from_numpy(np.ascontiguousarray(k, np.int32))
    ids = ids.contiguous()
    per_q = [k, skip, *extra_q]
    for j, t in enumerate(per_q):
        if t is not None:
            per_q[j] = t = _like_ids(t, ids)
            if t.shape != (Q,):
                raise ValueError("k, skip and truth must be [Q]")
    if dist is not None:
        dist = dist.contiguous()
        if dist.shape != ids.shape or dist.dtype != torch.float64 or dist.device != ids.device:
            raise ValueError("dist must be a float64 tensor shaped like ids")
    return (ids, per_q[0], per_q[1], dist, *per_q[2:]), (Q, ks)


def vote_curve_gpu(ids, k, labels, kcap: int, skip=None, truth=None, dist=None, hits=None, *,
                   weights: str = "uniform", score: bool = False, lists: bool = True):
    """vote_curve_cpu on the device (dmlp_vote_curve, or dmlp_vote_curve_weighted for a non-uniform
    `weights` or score=True; csrc/vote_curve.hip): ids [Q, kstride] int32, k / skip / truth [Q]
    int32, labels [N] int32 and dist (shaped like ids, float64) are torch tensors on one GPU (k may
    be a host array).  `hits`: an int64 [kcap] tensor there that the counts are ADDED to (a fresh
    zeroed one when truth is given without it), so a caller can sum over batches of rows without a
    copy back.  Bit-identical to the CPU's.  Asynchronous on the current stream."""
    torch = _torch()
    mode = _curve_weighted(weights, score, dist is not None)
    (ids, k, skip, dist, truth), (Q, ks) = _device_lists(ids, k, skip, dist, (truth,))
    dev = ids.device
    labels = _like_ids(labels, ids)
    kcap = _check_kcap(kcap)
    lab = torch.empty((Q, kcap), dtype=torch.int32, device=dev)
    lists = bool(lists) and dist is not None
    od = torch.empty((Q, kcap), dtype=torch.float64, device=dev) if lists else None
    oi = torch.empty((Q, kcap), dtype=torch.int32, device=dev) if lists else None
    if truth is not None:
        if hits is None:
            hits = torch.zeros(kcap, dtype=torch.int64, device=dev)
        elif hits.dtype != torch.int64 or tuple(hits.shape) != (kcap,) or hits.device != dev \
                or not hits.is_contiguous():
            raise ValueError("hits must be a contiguous int64 [kcap] tensor on the lists' device")
    else:
        hits = None
    lists = (od, oi) if lists else None
    if mode is None:
        _lib.check(_lib.lib().dmlp_vote_curve(_p(dist), _p(ids), ks, _p(k), Q, _p(skip),
                                              _p(labels), kcap, _p(lab), _p(od), _p(oi), _p(truth),
                                              _p(hits), _stream()), "vote curve")
        return lab, hits, lists
    sc = torch.empty((Q, kcap), dtype=torch.float64, device=dev) if score else None
    _lib.check(_lib.lib().dmlp_vote_curve_weighted(
        _p(dist), _p(ids), ks, _p(k), Q, _p(skip), _p(labels), mode, kcap, _p(lab), _p(sc), _p(od),
        _p(oi), _p(truth), _p(hits), _stream()), "weighted vote curve")
    return (lab, hits, lists, sc) if score else (lab, hits, lists)


def vote_scores_gpu(ids, k, labels, label_lo: int, nclass: int, weights: str = "uniform",
                    dist=None, skip=None):
    """vote_scores_cpu on the device (dmlp_vote_scores, csrc/vote_scores.hip): ids [Q, kstride]
    int32, k / skip [Q] int32, labels [N] int32 and dist (shaped like ids, float64) are torch
    tensors on one GPU (k may be a host array).  Returns (count [Q, nclass] int32, score [Q,
    nclass] float64, label [Q] int32) there, bit-identical to the CPU's.  Asynchronous on the
    current stream."""
    torch = _torch()
    label_lo, nclass, mode = _score_mode(label_lo, nclass, weights, dist is not None)
    (ids, k, skip, dist), (Q, ks) = _device_lists(ids, k, skip, dist)
    dev = ids.device
    labels = _like_ids(labels, ids)
    # every slot is written: no fill pass
    count = torch.empty((Q, nclass), dtype=torch.int32, device=dev)
    score = torch.empty((Q, nclass), dtype=torch.float64, device=dev)
    lab = torch.empty(Q, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().dmlp_vote_scores(_p(dist), _p(ids), ks, _p(k), Q, _p(skip), _p(labels),
                                           label_lo, nclass, mode, _p(count), _p(score), _p(lab),
                                           _stream()), "vote scores")
    return count, score, lab


def _means_gpu_args(ids, k, targets, weights, dist, skip, kcap=None):
    torch = _torch()
    (ids, k, skip, dist), _ = _device_lists(ids, k, skip, dist)
    if targets.dim() != 2 or targets.dtype != torch.float64 or targets.device != ids.device:
        raise ValueError("targets must be a float64 [N, T] tensor on the lists' device")
    T, mode, kcap = _means_args(targets.shape[1], weights, dist is not None, kcap)
    return ids, k, targets.contiguous(), dist, skip, T, mode, kcap


def neighbor_means_gpu(ids, k, targets, weights: str = "uniform", dist=None, skip=None):
    """neighbor_means_cpu on the device (dmlp_neighbor_means, csrc/neighbor_means.hip): ids [Q,
    kstride] int32, k / skip [Q] int32, targets [N, T] float64 and dist (shaped like ids, float64)
    are torch tensors on one GPU (k may be a host array).  Returns (mean [Q, T] float64, wsum [Q]
    float64, count [Q] int32) there, bit-identical to the CPU's.  Asynchronous on the current
    stream."""
    torch = _torch()
    ids, k, targets, dist, skip, T, mode, _ = _means_gpu_args(ids, k, targets, weights, dist, skip)
    Q, ks = ids.shape
    dev = ids.device
    # every slot is written: no fill pass
    mean = torch.empty((Q, T), dtype=torch.float64, device=dev)
    wsum = torch.empty(Q, dtype=torch.float64, device=dev)
    count = torch.empty(Q, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().dmlp_neighbor_means(_p(dist), _p(ids), ks, _p(k), Q, _p(skip),
                                              _p(targets), T, mode, _p(mean), _p(wsum), _p(count),
                                              _stream()), "neighbor means")
    return mean, wsum, count


def neighbor_means_curve_gpu(ids, k, targets, kcap: int, weights: str = "uniform", dist=None,
                             skip=None):
    """neighbor_means_curve_cpu on the device (dmlp_neighbor_means_curve): the mean over every
    prefix of the lists in one launch, float64 [Q, kcap, T] on the lists' GPU, bit-identical to the
    CPU's.  Arguments as for neighbor_means_gpu.  Asynchronous on the current stream."""
    torch = _torch()
    ids, k, targets, dist, skip, T, mode, kcap = _means_gpu_args(ids, k, targets, weights, dist,
                                                                 skip, kcap)
    Q, ks = ids.shape
    mean = torch.empty((Q, kcap, T), dtype=torch.float64, device=ids.device)
    _lib.check(_lib.lib().dmlp_neighbor_means_curve(_p(dist), _p(ids), ks, _p(k), Q, _p(skip),
                                                    _p(targets), T, mode, kcap, _p(mean),
                                                    _stream()), "neighbor means curve")
    return mean


# ---------------------------------------------------------------- radius search
def _radius_device_args(ds, Qx, r2):
    """(Qx, r2) of a device radius call: Qx a float64 [Q, A] tensor on the dataset's GPU (strided
    is fine), r2 a scalar, a host array or a tensor, float64 [Q] there afterwards.  ValueError for
    anything else."""
    torch = _torch()
    dev = ds.X.device
    if not torch.is_tensor(Qx) or Qx.dtype != torch.float64 or Qx.dim() != 2 or \
            Qx.shape[1] != ds.A or Qx.device != dev:
        raise ValueError("Qx must be a float64 [Q, A] tensor on the dataset's device")
    if ds.A < 1:
        raise ValueError("the dataset has no attributes")
    Q = Qx.shape[0]
    if torch.is_tensor(r2):
        if r2.dtype != torch.float64 or r2.device != dev:
            raise ValueError("r2 must be a float64 tensor on the dataset's device")
    else:
        r2 = np.asarray(r2, np.float64)
        if r2.ndim == 0:
            r2 = np.full(Q, float(r2), np.float64)
        r2 = torch.from_numpy(np.ascontiguousarray(r2)).to(dev)
    if tuple(r2.shape) != (Q,):
        raise ValueError("r2 must be a scalar or [Q]")
    return Qx.contiguous(), r2.contiguous()


def radius_count_gpu(ds: DeviceDataset, Qx, r2):
    """radius_count_cpu on the device (dmlp_radius_count, csrc/radius.hip): ds the prepared
    dataset, Qx a float64 [Q, A] tensor on its GPU, r2 the SQUARED radii (a scalar, a host array
    or a float64 [Q] tensor there).  Returns an int32 [Q] tensor there, the CPU's numbers.
    Asynchronous on the current stream."""
    torch = _torch()
    Qx, r2 = _radius_device_args(ds, Qx, r2)
    Q = Qx.shape[0]
    count = torch.zeros(Q, dtype=torch.int32, device=Qx.device)
    _lib.check(_lib.lib().dmlp_radius_count(_p(ds.X) if ds.N else None, ds.N, ds.A, _p(Qx), Q,
                                            _p(r2), _p(count), _stream()), "radius count")
    return count


def radius_gpu(ds: DeviceDataset, Qx, r2, sort: bool = True, stride=None, count=None):
    """radius_cpu on the device (dmlp_radius_fill, then dmlp_radius_sort unless sort=False):
    arguments as for radius_count_gpu, count its result when the caller has it.  stride=None: CSR
    (indptr int64 [Q + 1], dist [total], ids [total]) as tensors on the GPU, the prefix sum a
    torch.cumsum; stride=s: padded (dist [Q, s], ids [Q, s], count), pre-filled with (+inf, -1),
    which vote_scores_gpu and neighbor_means_gpu read with k = count.  Bit-identical to the CPU's.
    One host sync for the sizes (the total, or the largest count); a count above s or more than
    2^31 - 1 slots raise ValueError: callers batch."""
    torch = _torch()
    L = _lib.lib()
    Qx, r2 = _radius_device_args(ds, Qx, r2)
    Q = Qx.shape[0]
    dev = Qx.device
    if count is None:
        count = radius_count_gpu(ds, Qx, r2)
    if not torch.is_tensor(count) or count.dtype != torch.int32 or tuple(count.shape) != (Q,) \
            or count.device != dev:
        raise ValueError("count must be an int32 [Q] tensor on the dataset's device")
    count = count.contiguous()
    if stride is None:
        indptr = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
        torch.cumsum(count, 0, out=indptr[1:])
        total = int(indptr[Q].item()) if Q else 0
        span = _radius_layout(0, total, Q, None)
        off = indptr[:Q]
        d = torch.empty(total, dtype=torch.float64, device=dev)
        i = torch.empty(total, dtype=torch.int32, device=dev)
    else:
        span = _radius_layout(int(count.max().item()) if Q else 0, 0, Q, stride)
        off = torch.arange(Q, dtype=torch.int64, device=dev) * int(stride)
        d = torch.full((Q, int(stride)), float("inf"), dtype=torch.float64, device=dev)
        i = torch.full((Q, int(stride)), -1, dtype=torch.int32, device=dev)
    if Q and span and ds.N:
        _lib.check(L.dmlp_radius_fill(_p(ds.X), ds.N, ds.A, _p(Qx), Q, _p(r2), _p(count), _p(off),
                                      _p(d), _p(i), _stream()), "radius fill")
        if sort:
            nbytes = L.dmlp_radius_sort_bytes(span, Q)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(L.dmlp_radius_sort(_p(d), _p(i), _p(count), _p(off), Q, _p(ws), nbytes,
                                          _stream()), "radius sort")
    return (indptr, d, i) if stride is None else (d, i, count)


# ---------------------------------------------------------------- radius-graph components
def _device_rows(X, name: str = "X"):
    torch = _torch()
    if not torch.is_tensor(X) or X.dtype != torch.float64 or X.dim() != 2 or not X.is_cuda or \
            X.shape[1] < 1:
        raise ValueError(f"{name} must be a float64 [N, A] tensor on a GPU with A >= 1")
    return X.contiguous()


def radius_components_gpu(X, r2):
    """radius_components_cpu on the device (dmlp_radius_components, csrc/components.hip): X a
    float64 [N, A] tensor on a GPU (strided is fine), r2 a Python float.  Returns an int32 [N]
    tensor there, the CPU's integers.  One host sync, for the status word: a union-find walk that
    overran its bound raises RuntimeError."""
    torch = _torch()
    X = _device_rows(X)
    r2 = _components_r2(r2)
    N = X.shape[0]
    comp = torch.empty(N, dtype=torch.int32, device=X.device)
    if N:
        status = torch.zeros(1, dtype=torch.int32, device=X.device)
        _lib.check(_lib.lib().dmlp_radius_components(_p(X), N, X.shape[1], r2, _p(comp),
                                                     _p(status), _stream()), "radius components")
        if int(status.item()):
            raise RuntimeError("radius components: a union-find walk overran its step bound")
    return comp


def exact_nearest_gpu(X, Qx, qidx):
    """The nearest row of X (float64 [N, A] on a GPU) under (dist asc, id desc) for the rows qidx
    (int32 tensor, any order) of Qx (float64 [Q, A] there): dmlp_exact_topk at k = 1 on the raw
    device rows — no DeviceDataset, no screen.  Returns (dist float64 [Q], ids int32 [Q]) there,
    (+inf, -1) for the rows that are not listed and, with N = 0, for all.  knn_cpu at k = 1 is its
    CPU counterpart.  Asynchronous on the current stream."""
    torch = _torch()
    X, Qx = _device_rows(X), _device_rows(Qx, "Qx")
    if Qx.shape[1] != X.shape[1] or Qx.device != X.device:
        raise ValueError("Qx must have X's attribute count and device")
    Q = Qx.shape[0]
    if not torch.is_tensor(qidx) or qidx.dtype != torch.int32 or qidx.dim() != 1 or \
            qidx.device != X.device:
        raise ValueError("qidx must be an int32 [nb] tensor on X's device")
    qidx = qidx.contiguous()
    d = torch.full((Q,), float("inf"), dtype=torch.float64, device=X.device)
    i = torch.full((Q,), -1, dtype=torch.int32, device=X.device)
    if len(qidx) and X.shape[0]:
        qk = torch.ones(Q, dtype=torch.int32, device=X.device)
        _lib.check(_lib.lib().dmlp_exact_topk(_p(X), X.shape[0], X.shape[1], _p(Qx), _p(qidx),
                                              _p(qk), len(qidx), 1, _p(d), _p(i), 1, _stream()),
                   "exact nearest")
    return d, i


# ---------------------------------------------------------------- report text on the GPU
def format_report_dev(cs, qid_base: int = 0):
    """Render "Query <id> checksum: <u64>\\n" lines on the GPU.  Returns (device uint8 tensor,
    byte count); one host sync for the count."""
    torch = _torch()
    L = _lib.lib()
    cs = cs.contiguous()
    nq = cs.numel()
    if nq == 0:
        return torch.empty(0, dtype=torch.uint8, device=cs.device), 0
    off = torch.empty(L.dmlp_format_scratch(nq), dtype=torch.int64, device=cs.device)
    out = torch.empty(L.dmlp_format_bound(nq), dtype=torch.uint8, device=cs.device)
    _lib.check(L.dmlp_format_report(_p(cs), nq, qid_base, _p(off), _p(out), _stream()), "format")
    return out, int(off[nq].item())


_PINNED = {}


def _pinned_bytes(n: int):
    """Grow-only page-locked host staging buffer (D2H at DMA rate, no per-call pinning)."""
    torch = _torch()
    buf = _PINNED.get("report")
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(n, 1 << 20), dtype=torch.uint8).pin_memory()
        _PINNED["report"] = buf
    return buf


def format_report_gpu(cs, qid_base: int = 0):
    """Report bytes on the host: GPU formatter + one D2H into a pinned staging buffer.
    Returns a read-only memoryview valid until the next call (write it out or copy it)."""
    dev_text, n = format_report_dev(cs, qid_base)
    if n == 0:
        return memoryview(b"")
    host = _pinned_bytes(n)
    host[:n].copy_(dev_text[:n])
    return memoryview(host.numpy())[:n].toreadonly()
