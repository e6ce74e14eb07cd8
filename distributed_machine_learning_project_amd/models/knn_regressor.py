"""Model front-end: an estimator-style exact k-NN regressor.

    reg = KNNRegressor().fit(X, y)           # X [N, A] float64, y [N] or [N, T] float64, T <= 256
    dist, ids = reg.kneighbors(Q, k)         # k: int or per-query array
    pred = reg.predict(Q, k)                 # [Q] or [Q, T]: the mean of the neighbours' targets
    pred = reg.predict(Q, k, weights="inv_sqdist")   # neighbours weighted 1 / squared distance
    curve = reg.predict_curve(Q, kmax)       # [Q, kmax(, T)]: column k - 1 == predict(Q, k)
    curve = reg.loo_predict_curve(kmax)      # each dataset row's curve over its nearest OTHER rows
    sse, N = reg.loo_curve(kmax)             # leave-one-out squared error of every k <= kmax
    best_k, mse = reg.select_k(kmax)         # the smallest k with the least leave-one-out error
    pred = reg.radius_predict(Q, radius=r)   # the mean over the rows within r (or r2=: squared)

The search, update() and the row selection of the leave-one-out calls are KNNClassifier's, from
_knn_base.KNNBase (exact fp64 squared-L2 distances, neighbours ordered by (distance asc, id
desc)); a prediction is a function of the sorted lists the search leaves: the neighbour-mean kernel
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
from ..ops.knn import _torch
from ._knn_base import KNNBase


class KNNRegressor(KNNBase):
    def fit(self, X, y):
        self._fit_rows(X)
        y = np.asarray(y, np.float64)
        if y.ndim not in (1, 2) or y.shape[0] != self.X.shape[0]:
            raise ValueError("X must be [N, A] and y [N] or [N, T]")
        self._flat = y.ndim == 1        # predictions drop the target axis again
        self.y = np.ascontiguousarray(y[:, None] if self._flat else y)
        if not 1 <= self.y.shape[1] <= K.NEIGHBOR_MEANS_TMAX:
            raise ValueError(f"y must have between 1 and {K.NEIGHBOR_MEANS_TMAX} target columns")
        if self.on_gpu:
            torch = _torch()
            self._ds = self._prepare(torch.from_numpy(self.X).cuda())
            self._yd = torch.from_numpy(self.y).cuda()
        return self

    def _prepare(self, Xd):
        return K.prepare_dataset(Xd)

    def _shape(self, a):
        return a[..., 0] if self._flat else a

    # ------------------------------------------------------------ predictions
    def predict(self, Q, k, weights: str = "uniform"):
        """float64 [Q] (y fitted as [N]) or [Q, T]: the mean of the targets of the k nearest
        neighbours (k an int or a per-query array), uniform or weighted by 1 / squared distance.
        A row with k_q <= 0 is NaN.  Bit-identical on both devices."""
        K._weight_mode(weights, True)
        Q = np.ascontiguousarray(Q, np.float64)
        kk = self._k(Q, k)
        d, i = self._search(Q, kk)
        if self.on_gpu:
            mean = K.neighbor_means_gpu(i, kk, self._yd, weights, dist=d)[0]
        else:
            mean = K.neighbor_means_cpu(i, kk, self.y, weights, dist=d)[0]
        return self._shape(self._host(mean))

    def radius_predict(self, Q, radius=None, *, r2=None, weights: str = "uniform",
                       max_entries: int = 2 ** 26):
        """float64 [Q] or [Q, T]: the mean of the targets of every fitted row within `radius` (or
        the squared radius `r2`) of each query — predict(Q, radius_count(Q, ...), weights), bit
        for bit.  A query without a neighbour is NaN."""
        K._weight_mode(weights, True)
        out = []
        for _, _, d, i, c in self._radius_lists(Q, radius, r2, max_entries):
            if self.on_gpu:
                mean = K.neighbor_means_gpu(i, c, self._yd, weights, dist=d)[0]
            else:
                mean = K.neighbor_means_cpu(i, c, self.y, weights, dist=d)[0]
            out.append(self._host(mean))
        mean = np.concatenate(out) if out else np.empty((0, self.y.shape[1]), np.float64)
        return self._shape(mean)

    def _curve(self, d, i, kk, kmax, weights, skip=None):
        if self.on_gpu:
            return K.neighbor_means_curve_gpu(i, kk, self._yd, kmax, weights, dist=d, skip=skip)
        return K.neighbor_means_curve_cpu(i, kk, self.y, kmax, weights, dist=d, skip=skip)

    def predict_curve(self, Q, kmax: int, weights: str = "uniform"):
        """float64 [Q, kmax] or [Q, kmax, T]: column k - 1 is predict(Q, k, weights), bit for bit,
        from ONE search at kmax (columns past the dataset's size repeat the last one)."""
        K._weight_mode(weights, True)
        kmax = self._curve_kmax(kmax)
        Q = np.ascontiguousarray(Q, np.float64)
        kk = np.full(Q.shape[0], kmax, np.int32)
        d, i = self._search(Q, kk)
        return self._shape(self._host(self._curve(d, i, kk, kmax, weights)))

    # ------------------------------------------------------------ choosing k
    def _loo_batch(self, rows, kmax, weights):
        """The mean curve of the dataset rows `rows` over their nearest OTHER rows (_loo_lists, then
        the curve with skip = the row's own id): (means [R, kmax, T] — on the device for a GPU —,
        row ids)."""
        d, i, kk, idx, skip = self._loo_lists(rows, kmax)
        return self._curve(d, i, kk, kmax, weights, skip=skip), idx

    def loo_predict_curve(self, kmax: int, rows=None, weights: str = "uniform"):
        """float64 [R, kmax] or [R, kmax, T]: the prediction curve of the dataset rows `rows` (a
        slice or an index array; default: all) over their nearest OTHER rows; columns past N - 1
        repeat the last one.  kmax <= 255."""
        K._weight_mode(weights, True)
        kmax = self._loo_kmax(kmax)
        mean, _ = self._loo_batch(slice(None) if rows is None else rows, kmax, weights)
        return self._shape(self._host(mean))

    def loo_curve(self, kmax: int, weights: str = "uniform", batch_rows: int = 65536):
        """(sse float64 [kmax, T], N): sse[k - 1, t] = the squared error, summed over the rows, of
        target t predicted from each row's k nearest OTHER rows — leave-one-out, every k <= kmax
        from one self-join in batches of batch_rows rows.  Per batch only the [R, kmax, T] means
        cross back from a GPU; ops.knn.curve_sse's sums are added in batch order on the host, so
        both devices return the same bits."""
        K._weight_mode(weights, True)
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
