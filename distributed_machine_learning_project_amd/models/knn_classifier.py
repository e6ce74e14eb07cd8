"""Model front-ends: an estimator-style exact k-NN classifier and the serial KD-tree.

    clf = KNNClassifier().fit(X, y)          # X [N, A] float64, y [N] int
    dist, ids = clf.kneighbors(Q, k)         # k: int or per-query array
    labels = clf.predict(Q, k)               # majority vote, ties -> larger label
    cs = clf.checksums(Q, k)                 # reference FNV-1a report checksums
    proba = clf.predict_proba(Q, k)          # [Q, len(clf.classes_)]: class shares of the vote
    proba = clf.predict_proba(Q, k, weights="inv_sqdist")   # neighbours weighted 1 / squared distance
    labels = clf.predict(Q, k, weights="inv_sqdist")        # the weighted vote
    curve = clf.predict_curve(Q, kmax)       # [Q, kmax]: column k - 1 == predict(Q, k)
    dist, ids = clf.loo_kneighbors(kmax)     # neighbours of the dataset's own rows, self excluded
    hits, N = clf.loo_curve(kmax)            # leave-one-out hits of every k <= kmax
    best_k, acc = clf.select_k(kmax)         # the smallest k with the best leave-one-out accuracy
    best_k, acc = clf.select_k(kmax, weights="inv_sqdist")  # ... of the weighted vote (also on
                                             # predict_curve and loo_curve)
    count = clf.radius_count(Q, radius=r)    # fitted rows within r of each query (or r2=: squared)
    indptr, dist, ids = clf.radius_neighbors(Q, r2=r2)      # those rows in CSR, (dist asc, id desc)
    labels = clf.radius_predict(Q, r2=r2)    # == predict(Q, count); also radius_predict_proba

Semantics are the reference's: exact fp64 squared-L2 distances summed left to
right without FMA, neighbours ordered by (distance asc, id desc).  On a GPU the dataset is
prepared once at fit() (fp64 copy + bf16x3 MFMA fragments) and reused by every query batch;
on a CPU the native threaded brute force (or the KD-tree) runs.  The fitted rows, update(), the
search behind kneighbors() and the row selection of the leave-one-out calls are _knn_base.KNNBase's,
shared with KNNRegressor; this class adds the votes over the lists the search leaves.
"""
from __future__ import annotations

import numpy as np

from ..ops import knn as K
from ..ops.knn import _torch
from ._knn_base import KNNBase


class KNNClassifier(KNNBase):
    def fit(self, X, y):
        self._fit_rows(X)
        self.y = np.ascontiguousarray(y, np.int32)
        if self.y.shape[0] != self.X.shape[0]:
            raise ValueError("X must be [N, A] and y [N]")
        lo = int(self.y.min()) if len(self.y) else 0
        hi = int(self.y.max()) + 1 if len(self.y) else 1
        self._label_range = (lo, hi)
        if self.on_gpu:
            torch = _torch()
            self._yd = torch.from_numpy(self.y).cuda()
            self._ds = self._prepare(torch.from_numpy(self.X).cuda())
        return self

    def _prepare(self, Xd):
        return K.prepare_dataset(Xd, self._yd, self._label_range)

    def _run(self, Q, k):
        """(labels, checksums) of the majority vote: on a GPU the vote and the checksum are fused
        into the search (ONE knn_gpu call, nothing but the two results crosses back)."""
        Q = np.ascontiguousarray(Q, np.float64)
        kk = self._k(Q, k)
        if self.on_gpu:
            r = K.knn_gpu(self._ds, _torch().from_numpy(Q).cuda(), kk, finalize=True,
                          exact=self.exact)
            return r.label.cpu().numpy(), r.checksum.cpu().numpy().view(np.uint64)
        return K.finalize_cpu(self._search(Q, kk)[1], kk, self.y)

    def predict(self, Q, k, weights: str = "uniform"):
        """The vote of the k nearest neighbours.  weights="inv_sqdist": the class with the largest
        (score, count, label) of predict_proba's weighted scores instead of the majority."""
        if weights == "uniform":
            return self._run(Q, k)[0]
        return self._host(self._scores(Q, k, weights)[2])

    def checksums(self, Q, k):
        return self._run(Q, k)[1]

    # ------------------------------------------------------------ class scores
    # Per-class votes are a function of the lists the search leaves on the device: one search
    # without the fused vote, then the class-score kernel (csrc/vote_scores.hip;
    # dmlp_cpu_vote_scores on a CPU).
    @property
    def classes_(self):
        """np.arange(lo, hi) over the fitted labels' range: the columns of predict_proba."""
        lo, hi = self._label_range
        if hi - lo > K.VOTE_SCORES_CMAX:
            raise ValueError(f"the labels span {hi - lo} values: class scores take at most "
                             f"{K.VOTE_SCORES_CMAX}")
        return np.arange(lo, hi)

    def _scores(self, Q, k, weights):
        """(count [Q, C] int32, score [Q, C] float64, label [Q] int32) of the k nearest neighbours,
        on the device for a GPU (_host brings one back)."""
        K._weight_mode(weights, True)
        lo, nclass = int(self.classes_[0]), len(self.classes_)
        Q = np.ascontiguousarray(Q, np.float64)
        kk = self._k(Q, k)
        d, i = self._search(Q, kk)
        if self.on_gpu:
            return K.vote_scores_gpu(i, kk, self._yd, lo, nclass, weights, dist=d)
        return K.vote_scores_cpu(i, kk, self.y, lo, nclass, weights, dist=d)

    def predict_proba(self, Q, k, weights: str = "uniform"):
        """float64 [Q, len(classes_)]: the share of each class among the k nearest neighbours (k an
        int or a per-query array).  weights="inv_sqdist" weighs a neighbour by 1 / d, d the
        SQUARED distance the lists hold (not the 1 / distance of some libraries); a query that
        coincides with training rows gives probability to their classes only.  Rows sum to 1; a
        row without neighbours (k_q <= 0) is all zeros.  Bit-identical on both devices."""
        cnt, sc, _ = self._scores(Q, k, weights)
        # only the scores cross back, and the counts when a row's scores sum to 0
        return K.class_proba(self._host(sc), lambda: self._host(cnt))

    # ------------------------------------------------------------ radius votes
    def _radius_scores(self, Q, radius, r2, weights, max_entries, want):
        """Per batch of the radius search's padded lists (KNNBase._radius_lists) the class-score
        kernel at k = count; `want` picks what comes back to the host from (count, score, label)."""
        K._weight_mode(weights, True)
        lo, nclass = int(self.classes_[0]), len(self.classes_)
        out = []
        for _, _, d, i, c in self._radius_lists(Q, radius, r2, max_entries):
            if self.on_gpu:
                res = K.vote_scores_gpu(i, c, self._yd, lo, nclass, weights, dist=d)
            else:
                res = K.vote_scores_cpu(i, c, self.y, lo, nclass, weights, dist=d)
            out.append(want(res))
        return out

    def radius_predict(self, Q, radius=None, *, r2=None, weights: str = "uniform",
                       max_entries: int = 2 ** 26):
        """int32 [Q]: the vote of every fitted row within `radius` (or the squared radius `r2`) of
        each query — predict(Q, radius_count(Q, ...), weights), bit for bit.  A query without a
        neighbour predicts -1.  The label range limit is predict_proba's."""
        out = self._radius_scores(Q, radius, r2, weights, max_entries,
                                  lambda r: self._host(r[2]))
        return np.concatenate(out) if out else np.empty(0, np.int32)

    def radius_predict_proba(self, Q, radius=None, *, r2=None, weights: str = "uniform",
                             max_entries: int = 2 ** 26):
        """float64 [Q, len(classes_)]: predict_proba over the rows within the radius, bit for bit
        its result at k = radius_count(Q, ...).  A query without a neighbour is all zeros."""
        out = self._radius_scores(
            Q, radius, r2, weights, max_entries,
            lambda r: K.class_proba(self._host(r[1]), lambda: self._host(r[0])))
        return np.concatenate(out) if out else np.empty((0, len(self.classes_)), np.float64)

    # ------------------------------------------------------------ choosing k
    # The lists are sorted, so the vote for every k <= kmax is a function of one list: one search
    # at kmax, then the vote-curve kernel (csrc/vote_curve.hip; dmlp_cpu_vote_curve on a CPU).  A
    # non-uniform `weights` takes the weighted curve of the same file, which reads the search's
    # distances as well; no label range is taken, so predict_proba's limit does not apply.
    def predict_curve(self, Q, kmax: int, weights: str = "uniform"):
        """int32 [Q, kmax]: column k - 1 is predict(Q, k, weights), bit for bit, from ONE search at
        kmax."""
        K._weight_mode(weights, True)
        kmax = self._curve_kmax(kmax)
        Q = np.ascontiguousarray(Q, np.float64)
        kk = np.full(Q.shape[0], kmax, np.int32)
        d, i = self._search(Q, kk)
        dist = None if weights == "uniform" else d
        if self.on_gpu:
            return K.vote_curve_gpu(i, kk, self._yd, kmax, dist=dist, weights=weights,
                                    lists=False)[0].cpu().numpy()
        return K.vote_curve_cpu(i, kk, self.y, kmax, dist=dist, weights=weights, lists=False)[0]

    def _loo_batch(self, rows, kmax, lists, hits=None, weights="uniform"):
        """The vote curve of the dataset rows `rows` over their nearest OTHER rows (_loo_lists, then
        the curve with skip = the row's own id): (labels, hits, lists), on the device for a GPU —
        the kept lists when `lists`, else the hits against the rows' own labels.  A non-uniform
        `weights` sends the distances to the kernel either way."""
        d, i, kk, idx, skip = self._loo_lists(rows, kmax)
        dist = d if lists or weights != "uniform" else None
        if self.on_gpu:
            truth = None if lists else self._yd[skip.long()]
            return K.vote_curve_gpu(i, kk, self._yd, kmax, skip=skip, truth=truth, dist=dist,
                                    hits=hits, weights=weights, lists=lists)
        truth = None if lists else self.y[idx]
        return K.vote_curve_cpu(i, kk, self.y, kmax, skip=skip, truth=truth, dist=dist, hits=hits,
                                weights=weights, lists=lists)

    def loo_kneighbors(self, kmax: int, rows=None):
        """(dist, ids) [R, kmax]: the kmax nearest neighbours of the dataset rows `rows` (a slice
        or an index array; default: all) with the row itself left out, padded with (+inf, -1)
        when fewer than kmax other points exist.  kmax <= 255."""
        kmax = self._loo_kmax(kmax)
        _, _, (d, i) = self._loo_batch(slice(None) if rows is None else rows, kmax, lists=True)
        return self._host(d), self._host(i)

    def loo_curve(self, kmax: int, batch_rows: int = 65536, weights: str = "uniform"):
        """(hits int64 [kmax], N): hits[k - 1] = the rows whose k nearest OTHER rows vote their own
        label (under `weights`, as predict does) — leave-one-out, every k <= kmax from one
        self-join in batches of batch_rows rows.  On a GPU the counts stay on the device over the
        batches: one copy back at the end."""
        K._weight_mode(weights, True)
        kmax = self._loo_kmax(kmax)
        N = self.X.shape[0]
        step = max(1, int(batch_rows))
        hits = None
        for a in range(0, N, step):
            hits = self._loo_batch(slice(a, min(N, a + step)), kmax, lists=False, hits=hits,
                                   weights=weights)[1]
        if hits is None:
            return np.zeros(kmax, np.int64), N
        return self._host(hits), N

    def select_k(self, kmax: int, weights: str = "uniform"):
        """(best_k, accuracy float64 [kmax]): leave-one-out accuracy of every k <= kmax under
        `weights` and the smallest k that reaches the best one (chosen on the integer hit
        counts)."""
        hits, N = self.loo_curve(kmax, weights=weights)
        if N == 0:
            raise ValueError("select_k needs a fitted, non-empty dataset")
        return int(np.argmax(hits)) + 1, hits.astype(np.float64) / N


class KDTree:
    """Serial exact KD-tree (bench.debug B0): median split on axis depth % A, near side first,
    far side visited when the split-plane bound can still tie the current k-th distance."""

    def __init__(self, X):
        self.X = np.ascontiguousarray(X, np.float64)

    def query(self, Q, k):
        Q = np.ascontiguousarray(Q, np.float64)
        kk = np.full(Q.shape[0], int(k), np.int32) if np.isscalar(k) else np.asarray(k, np.int32)
        return K.knn_cpu(self.X, Q, kk, method="kdtree")
