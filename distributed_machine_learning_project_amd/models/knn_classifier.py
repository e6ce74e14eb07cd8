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

Semantics are the reference's: exact fp64 squared-L2 distances summed left to
right without FMA, neighbours ordered by (distance asc, id desc).  On a GPU the dataset is
prepared once at fit() (fp64 copy + bf16x3 MFMA fragments) and reused by every query batch;
on a CPU the native threaded brute force (or the KD-tree) runs.
"""
from __future__ import annotations

import numpy as np

from ..ops import knn as K


def _torch():
    import torch
    return torch


class KNNClassifier:
    def __init__(self, device: str = "auto", exact: bool = False, cpu_method: str = "brute"):
        torch = _torch()
        self.on_gpu = device == "gpu" or (device == "auto" and torch.cuda.is_available())
        self.exact = exact
        self.cpu_method = cpu_method
        self._ds = None

    def fit(self, X, y):
        self.X = np.ascontiguousarray(X, np.float64)
        self.y = np.ascontiguousarray(y, np.int32)
        if self.X.ndim != 2 or self.y.shape[0] != self.X.shape[0]:
            raise ValueError("X must be [N, A] and y [N]")
        lo = int(self.y.min()) if len(self.y) else 0
        hi = int(self.y.max()) + 1 if len(self.y) else 1
        self._label_range = (lo, hi)
        if self.on_gpu:
            torch = _torch()
            self._ds = K.prepare_dataset(torch.from_numpy(self.X).cuda(),
                                         torch.from_numpy(self.y).cuda(), (lo, hi))
        return self

    def update(self, updates):
        """Apply Update records (common.h:22-25) to the fitted dataset: rows are replaced in the
        host copy and, on a GPU, scattered into the device copy, after which the screen layout
        (centering, bf16 fragments, norms) is rebuilt so later queries stay exact."""
        updates = list(updates)
        if not updates:
            return self
        for u in updates:
            if not 0 <= u.id < self.X.shape[0] or len(u.new_attrs) != self.X.shape[1]:
                raise ValueError(f"update {u.id}: id out of range or wrong attribute count")
            self.X[u.id] = np.asarray(u.new_attrs, np.float64)
        if self.on_gpu:
            torch = _torch()
            ids = np.array(sorted({u.id for u in updates}), np.int64)
            Xd = self._ds.X
            Xd[torch.from_numpy(ids).to(Xd.device)] = torch.from_numpy(self.X[ids]).to(Xd.device)
            self._ds = K.prepare_dataset(Xd, self._ds.labels, (self._ds.label_lo, self._ds.label_hi))
        return self

    def _k(self, Q, k):
        if np.isscalar(k):
            return np.full(Q.shape[0], int(k), np.int32)
        return np.ascontiguousarray(k, np.int32)

    def _run(self, Q, k, finalize):
        Q = np.ascontiguousarray(Q, np.float64)
        kk = self._k(Q, k)
        if self.on_gpu:
            torch = _torch()
            r = K.knn_gpu(self._ds, torch.from_numpy(Q).cuda(), kk, finalize=finalize,
                          exact=self.exact)
            d, i = r.dist.cpu().numpy(), r.ids.cpu().numpy()
            lab = r.label.cpu().numpy() if r.label is not None else None
            cs = r.checksum.cpu().numpy().view(np.uint64) if r.checksum is not None else None
            return d, i, lab, cs, kk
        d, i = K.knn_cpu(self.X, Q, kk, method=self.cpu_method)
        lab = cs = None
        if finalize:
            lab, cs = K.finalize_cpu(i, kk, self.y)
        return d, i, lab, cs, kk

    def kneighbors(self, Q, k):
        """(dist [Q, kmax], ids [Q, kmax]); row q is valid up to k_q, padded with (+inf, -1)."""
        d, i, _, _, _ = self._run(Q, k, finalize=False)
        return d, i

    def predict(self, Q, k, weights: str = "uniform"):
        """The vote of the k nearest neighbours.  weights="inv_sqdist": the class with the largest
        (score, count, label) of predict_proba's weighted scores instead of the majority."""
        if weights == "uniform":
            return self._run(Q, k, finalize=True)[2]
        return self._host(self._scores(Q, k, weights)[2])

    def checksums(self, Q, k):
        return self._run(Q, k, finalize=True)[3]

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
        if weights not in K.VOTE_WEIGHTS:
            raise ValueError(f"weights must be one of {sorted(K.VOTE_WEIGHTS)}, not {weights!r}")
        lo, nclass = int(self.classes_[0]), len(self.classes_)
        Q = np.ascontiguousarray(Q, np.float64)
        kk = self._k(Q, k)
        if self.on_gpu:
            torch = _torch()
            r = K.knn_gpu(self._ds, torch.from_numpy(Q).cuda(), kk, finalize=False,
                          exact=self.exact)
            return K.vote_scores_gpu(r.ids, kk, self._ds.labels, lo, nclass, weights, dist=r.dist)
        d, i = K.knn_cpu(self.X, Q, kk, method=self.cpu_method)
        return K.vote_scores_cpu(i, kk, self.y, lo, nclass, weights, dist=d)

    def _host(self, a):
        return a.cpu().numpy() if self.on_gpu else a

    def predict_proba(self, Q, k, weights: str = "uniform"):
        """float64 [Q, len(classes_)]: the share of each class among the k nearest neighbours (k an
        int or a per-query array).  weights="inv_sqdist" weighs a neighbour by 1 / d, d the
        SQUARED distance the lists hold (not the 1 / distance of some libraries); a query that
        coincides with training rows gives probability to their classes only.  Rows sum to 1; a
        row without neighbours (k_q <= 0) is all zeros.  Bit-identical on both devices."""
        cnt, sc, _ = self._scores(Q, k, weights)
        # only the scores cross back, and the counts when a row's scores sum to 0
        return K.class_proba(self._host(sc), lambda: self._host(cnt))

    # ------------------------------------------------------------ choosing k
    # The lists are sorted, so the vote for every k <= kmax is a function of one list: one search
    # at kmax, then the vote-curve kernel (csrc/vote_curve.hip; dmlp_cpu_vote_curve on a CPU).
    def predict_curve(self, Q, kmax: int):
        """int32 [Q, kmax]: column k - 1 is predict(Q, k), bit for bit, from ONE search at kmax."""
        kmax = int(kmax)
        if not 1 <= kmax <= K.VOTE_CURVE_KMAX:
            raise ValueError(f"kmax must be in [1, {K.VOTE_CURVE_KMAX}]")
        Q = np.ascontiguousarray(Q, np.float64)
        kk = np.full(Q.shape[0], kmax, np.int32)
        if self.on_gpu:
            torch = _torch()
            r = K.knn_gpu(self._ds, torch.from_numpy(Q).cuda(), kk, finalize=False,
                          exact=self.exact)
            return K.vote_curve_gpu(r.ids, kk, self._ds.labels, kmax)[0].cpu().numpy()
        _, i = K.knn_cpu(self.X, Q, kk, method=self.cpu_method)
        return K.vote_curve_cpu(i, kk, self.y, kmax)[0]

    def _loo_kmax(self, kmax):
        kmax = int(kmax)
        if not 1 <= kmax < K.VOTE_CURVE_KMAX:  # the search runs at kmax + 1: the row itself
            raise ValueError(f"kmax must be in [1, {K.VOTE_CURVE_KMAX - 1}]")
        return kmax

    def _loo_batch(self, rows, kmax, lists, hits=None):
        """Dataset rows `rows` (a slice with step 1, or an int array) as queries at k = min(kmax +
        1, N), then the curve with skip = the row's own id: (labels, hits, lists), on the device
        for a GPU.  With duplicates the row need not lead its own list, and when more than kmax +
        1 points tie at distance 0 it may be absent: the first kmax entries are then the answer,
        which is what dropping the id wherever it sits (or nowhere) gives."""
        N = self.X.shape[0]
        ks = max(1, min(kmax + 1, N))
        if isinstance(rows, slice):
            idx = np.arange(*rows.indices(N), dtype=np.int32)
        else:
            idx = np.ascontiguousarray(rows, np.int64)
            if idx.ndim != 1 or (len(idx) and (idx.min() < -N or idx.max() >= N)):
                raise ValueError("rows must be a slice or a 1-d array of row ids")
            idx = np.where(idx < 0, idx + N, idx).astype(np.int32)
        kk = np.full(len(idx), ks, np.int32)
        if self.on_gpu:
            torch = _torch()
            ds = self._ds
            if isinstance(rows, slice) and rows.indices(N)[2] == 1:
                Qd = ds.X[idx[0]:idx[0] + len(idx)] if len(idx) else ds.X[:0]
            else:  # a device-to-device gather: no host round trip
                Qd = ds.X.index_select(0, torch.from_numpy(idx.astype(np.int64)).to(ds.X.device))
            r = K.knn_gpu(ds, Qd, kk, finalize=False, exact=self.exact, kstride=ks)
            me = torch.from_numpy(idx).to(ds.X.device)
            return K.vote_curve_gpu(r.ids, kk, ds.labels, kmax, skip=me,
                                    truth=ds.labels[me.long()] if not lists else None,
                                    dist=r.dist if lists else None, hits=hits)
        d, i = K.knn_cpu(self.X, self.X[idx], kk, kstride=ks, method=self.cpu_method)
        return K.vote_curve_cpu(i, kk, self.y, kmax, skip=idx,
                                truth=self.y[idx] if not lists else None,
                                dist=d if lists else None, hits=hits)

    def loo_kneighbors(self, kmax: int, rows=None):
        """(dist, ids) [R, kmax]: the kmax nearest neighbours of the dataset rows `rows` (a slice
        or an index array; default: all) with the row itself left out, padded with (+inf, -1)
        when fewer than kmax other points exist.  kmax <= 255."""
        kmax = self._loo_kmax(kmax)
        _, _, (d, i) = self._loo_batch(slice(None) if rows is None else rows, kmax, lists=True)
        if self.on_gpu:
            return d.cpu().numpy(), i.cpu().numpy()
        return d, i

    def loo_curve(self, kmax: int, batch_rows: int = 65536):
        """(hits int64 [kmax], N): hits[k - 1] = the rows whose k nearest OTHER rows vote their own
        label — leave-one-out, every k <= kmax from one self-join in batches of batch_rows rows.
        On a GPU the counts stay on the device over the batches: one copy back at the end."""
        kmax = self._loo_kmax(kmax)
        N = self.X.shape[0]
        step = max(1, int(batch_rows))
        hits = None
        for a in range(0, N, step):
            _, hits, _ = self._loo_batch(slice(a, min(N, a + step)), kmax, lists=False, hits=hits)
        if hits is None:
            return np.zeros(kmax, np.int64), N
        return (hits.cpu().numpy() if self.on_gpu else hits), N

    def select_k(self, kmax: int):
        """(best_k, accuracy float64 [kmax]): leave-one-out accuracy of every k <= kmax and the
        smallest k that reaches the best one (chosen on the integer hit counts)."""
        hits, N = self.loo_curve(kmax)
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
