"""Model front-end: an estimator-style exact k-NN regressor.

    reg = KNNRegressor().fit(X, y)           # X [N, A] float64, y [N] or [N, T] float64, T <= 256
    dist, ids = reg.kneighbors(Q, k)         # k: int or per-query array
    pred = reg.predict(Q, k)                 # [Q] or [Q, T]: the mean of the neighbours' targets
    pred = reg.predict(Q, k, weights="inv_sqdist")   # neighbours weighted 1 / squared distance
    curve = reg.predict_curve(Q, kmax)       # [Q, kmax(, T)]: column k - 1 == predict(Q, k)
    curve = reg.loo_predict_curve(kmax)      # each dataset row's curve over its nearest OTHER rows
    sse, N = reg.loo_curve(kmax)             # leave-one-out squared error of every k <= kmax
    best_k, mse = reg.select_k(kmax)         # the smallest k with the least leave-one-out error

The search is KNNClassifier's (exact fp64 squared-L2 distances, neighbours ordered by (distance
asc, id desc)); a prediction is a function of the sorted lists it leaves: the neighbour-mean kernel
(csrc/neighbor_means.hip; dmlp_cpu_neighbor_means on a CPU) sums the targets in list order, left to
right, without FMA, so predictions are bit-identical on both devices.  weights="inv_sqdist" weighs
a neighbour by 1 / d, d the SQUARED distance the lists hold (computed as d_ref / d, d_ref the
nearest kept neighbour's, so nothing overflows); a query that coincides with training rows
predicts the mean of those rows.  On a GPU the dataset is prepared once at fit() without labels,
and the targets live on the device beside it.
"""
from __future__ import annotations

import numpy as np

from ..ops import knn as K


def _torch():
    import torch
    return torch


class KNNRegressor:
    def __init__(self, device: str = "auto", exact: bool = False, cpu_method: str = "brute"):
        torch = _torch()
        self.on_gpu = device == "gpu" or (device == "auto" and torch.cuda.is_available())
        self.exact = exact
        self.cpu_method = cpu_method
        self._ds = None

    def fit(self, X, y):
        self.X = np.ascontiguousarray(X, np.float64)
        y = np.asarray(y, np.float64)
        if self.X.ndim != 2 or y.ndim not in (1, 2) or y.shape[0] != self.X.shape[0]:
            raise ValueError("X must be [N, A] and y [N] or [N, T]")
        self._flat = y.ndim == 1        # predictions drop the target axis again
        self.y = np.ascontiguousarray(y[:, None] if self._flat else y)
        if not 1 <= self.y.shape[1] <= K.NEIGHBOR_MEANS_TMAX:
            raise ValueError(f"y must have between 1 and {K.NEIGHBOR_MEANS_TMAX} target columns")
        if self.on_gpu:
            torch = _torch()
            self._ds = K.prepare_dataset(torch.from_numpy(self.X).cuda())
            self._yd = torch.from_numpy(self.y).cuda()
        return self

    def update(self, updates):
        """Apply Update records (common.h:22-25) to the fitted dataset: rows are replaced in the
        host copy and, on a GPU, scattered into the device copy, after which the screen layout
        is rebuilt so later queries stay exact.  The targets stay as fitted."""
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
            self._ds = K.prepare_dataset(Xd)
        return self

    # ------------------------------------------------------------ the search
    def _k(self, Q, k):
        if np.isscalar(k):
            return np.full(Q.shape[0], int(k), np.int32)
        return np.ascontiguousarray(k, np.int32)

    def _search(self, Qx, kk, kstride=None):
        """(dist, ids) of the queries Qx — a host array, or on a GPU a device tensor —, on the
        device for a GPU."""
        if self.on_gpu:
            torch = _torch()
            Qd = Qx if torch.is_tensor(Qx) else torch.from_numpy(Qx).cuda()
            r = K.knn_gpu(self._ds, Qd, kk, finalize=False, exact=self.exact, kstride=kstride)
            return r.dist, r.ids
        return K.knn_cpu(self.X, Qx, kk, kstride=kstride, method=self.cpu_method)

    def _host(self, a):
        return a.cpu().numpy() if self.on_gpu else a

    def _shape(self, a):
        return a[..., 0] if self._flat else a

    @staticmethod
    def _weights(weights):
        if weights not in K.VOTE_WEIGHTS:
            raise ValueError(f"weights must be one of {sorted(K.VOTE_WEIGHTS)}, not {weights!r}")
        return weights

    def kneighbors(self, Q, k):
        """(dist [Q, kmax], ids [Q, kmax]); row q is valid up to k_q, padded with (+inf, -1)."""
        Q = np.ascontiguousarray(Q, np.float64)
        d, i = self._search(Q, self._k(Q, k))
        return self._host(d), self._host(i)

    # ------------------------------------------------------------ predictions
    def predict(self, Q, k, weights: str = "uniform"):
        """float64 [Q] (y fitted as [N]) or [Q, T]: the mean of the targets of the k nearest
        neighbours (k an int or a per-query array), uniform or weighted by 1 / squared distance.
        A row with k_q <= 0 is NaN.  Bit-identical on both devices."""
        weights = self._weights(weights)
        Q = np.ascontiguousarray(Q, np.float64)
        kk = self._k(Q, k)
        d, i = self._search(Q, kk)
        if self.on_gpu:
            mean = K.neighbor_means_gpu(i, kk, self._yd, weights, dist=d)[0]
        else:
            mean = K.neighbor_means_cpu(i, kk, self.y, weights, dist=d)[0]
        return self._shape(self._host(mean))

    def _curve(self, d, i, kk, kmax, weights, skip=None):
        if self.on_gpu:
            return K.neighbor_means_curve_gpu(i, kk, self._yd, kmax, weights, dist=d, skip=skip)
        return K.neighbor_means_curve_cpu(i, kk, self.y, kmax, weights, dist=d, skip=skip)

    def predict_curve(self, Q, kmax: int, weights: str = "uniform"):
        """float64 [Q, kmax] or [Q, kmax, T]: column k - 1 is predict(Q, k, weights), bit for bit,
        from ONE search at kmax (columns past the dataset's size repeat the last one)."""
        weights = self._weights(weights)
        kmax = int(kmax)
        if not 1 <= kmax <= K.VOTE_CURVE_KMAX:
            raise ValueError(f"kmax must be in [1, {K.VOTE_CURVE_KMAX}]")
        Q = np.ascontiguousarray(Q, np.float64)
        kk = np.full(Q.shape[0], kmax, np.int32)
        d, i = self._search(Q, kk)
        return self._shape(self._host(self._curve(d, i, kk, kmax, weights)))

    # ------------------------------------------------------------ choosing k
    def _loo_kmax(self, kmax):
        kmax = int(kmax)
        if not 1 <= kmax < K.VOTE_CURVE_KMAX:  # the search runs at kmax + 1: the row itself
            raise ValueError(f"kmax must be in [1, {K.VOTE_CURVE_KMAX - 1}]")
        return kmax

    def _loo_batch(self, rows, kmax, weights):
        """Dataset rows `rows` (a slice with step 1, or an int array) as queries at k = min(kmax +
        1, N), then the mean curve with skip = the row's own id: (means [R, kmax, T] — on the
        device for a GPU —, row ids).  With duplicates the row need not lead its own list, and
        when more than kmax + 1 points tie at distance 0 it may be absent: the first kmax entries
        are then the answer, which is what dropping the id wherever it sits (or nowhere) gives."""
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
            Xd = self._ds.X
            if isinstance(rows, slice) and rows.indices(N)[2] == 1:
                Qd = Xd[idx[0]:idx[0] + len(idx)] if len(idx) else Xd[:0]
            else:  # a device-to-device gather: no host round trip
                Qd = Xd.index_select(0, torch.from_numpy(idx.astype(np.int64)).to(Xd.device))
            d, i = self._search(Qd, kk, kstride=ks)
            skip = torch.from_numpy(idx).to(Xd.device)
        else:
            d, i = self._search(self.X[idx], kk, kstride=ks)
            skip = idx
        return self._curve(d, i, kk, kmax, weights, skip=skip), idx

    def loo_predict_curve(self, kmax: int, rows=None, weights: str = "uniform"):
        """float64 [R, kmax] or [R, kmax, T]: the prediction curve of the dataset rows `rows` (a
        slice or an index array; default: all) over their nearest OTHER rows; columns past N - 1
        repeat the last one.  kmax <= 255."""
        weights = self._weights(weights)
        kmax = self._loo_kmax(kmax)
        mean, _ = self._loo_batch(slice(None) if rows is None else rows, kmax, weights)
        return self._shape(self._host(mean))

    def loo_curve(self, kmax: int, weights: str = "uniform", batch_rows: int = 65536):
        """(sse float64 [kmax, T], N): sse[k - 1, t] = the squared error, summed over the rows, of
        target t predicted from each row's k nearest OTHER rows — leave-one-out, every k <= kmax
        from one self-join in batches of batch_rows rows.  Per batch only the [R, kmax, T] means
        cross back from a GPU; ops.knn.curve_sse's sums are added in batch order on the host, so
        both devices return the same bits."""
        weights = self._weights(weights)
        kmax = self._loo_kmax(kmax)
        N, T = self.y.shape
        step = max(1, int(batch_rows))
        sse = np.zeros((kmax, T), np.float64)
        for a in range(0, N, step):
            mean, idx = self._loo_batch(slice(a, min(N, a + step)), kmax, weights)
            sse = sse + K.curve_sse(self._host(mean), self.y[idx])
        return sse, N

    def select_k(self, kmax: int, weights: str = "uniform"):
        """(best_k, mse float64 [kmax]): the leave-one-out mean squared error of every k <= kmax
        over all rows and targets, and the smallest k with the smallest summed squared error."""
        if self.X.shape[0] < 2:
            raise ValueError("select_k needs at least two fitted rows")
        sse, N = self.loo_curve(kmax, weights=weights)
        tot = sse.sum(axis=1)
        return int(np.argmin(tot)) + 1, tot / (N * sse.shape[1])
