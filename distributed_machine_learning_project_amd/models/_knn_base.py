"""What the k-NN estimators share: the fitted rows on the host and, on a GPU, on the device; Update
records; the exact search (ops.knn.knn_gpu without the fused vote on a GPU, knn_cpu otherwise); and
the front of every leave-one-out call, which turns dataset rows into queries against the dataset
itself.  An estimator adds fit(), a one-line _prepare() and the kernels that read the sorted lists
(votes for KNNClassifier, neighbour means for KNNRegressor).
"""
from __future__ import annotations

import numpy as np

from ..ops import knn as K
from ..ops.knn import _torch


class KNNBase:
    def __init__(self, device: str = "auto", exact: bool = False, cpu_method: str = "brute"):
        self.on_gpu = device == "gpu" or (device == "auto" and _torch().cuda.is_available())
        self.exact = exact
        self.cpu_method = cpu_method
        self._ds = None

    def _fit_rows(self, X):
        self.X = np.ascontiguousarray(X, np.float64)
        if self.X.ndim != 2:
            raise ValueError("X must be [N, A]")

    def _prepare(self, Xd):
        """The DeviceDataset of the device rows Xd, with whatever the estimator keeps beside them."""
        raise NotImplementedError

    def update(self, updates):
        """Apply Update records (common.h:22-25) to the fitted dataset: rows are replaced in the
        host copy and, on a GPU, scattered into the device copy, after which the screen layout
        (centering, bf16 fragments, norms) is rebuilt so later queries stay exact.  Labels and
        targets stay as fitted."""
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
            self._ds = self._prepare(Xd)
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

    def kneighbors(self, Q, k):
        """(dist [Q, kmax], ids [Q, kmax]); row q is valid up to k_q, padded with (+inf, -1)."""
        Q = np.ascontiguousarray(Q, np.float64)
        d, i = self._search(Q, self._k(Q, k))
        return self._host(d), self._host(i)

    # ------------------------------------------------------------ curves and leave-one-out
    def _curve_kmax(self, kmax):
        return K._check_kcap(kmax, "kmax")

    def _loo_kmax(self, kmax):
        kmax = int(kmax)
        if not 1 <= kmax < K.VOTE_CURVE_KMAX:  # the search runs at kmax + 1: the row itself
            raise ValueError(f"kmax must be in [1, {K.VOTE_CURVE_KMAX - 1}]")
        return kmax

    def _loo_lists(self, rows, kmax):
        """Dataset rows `rows` (a slice or an int array, negative ids counting from the end) as
        queries at k = min(kmax + 1, N): (dist, ids, k, row ids, skip) — the lists at stride k, and
        the row ids again as the curve kernels' skip argument; dist, ids and skip on the device for
        a GPU.  A curve with skip = the row's own id is the leave-one-out answer: with duplicates
        the row need not lead its own list, and when more than kmax + 1 points tie at distance 0 it
        may be absent: the first kmax entries are then the answer, which is what dropping the id
        wherever it sits (or nowhere) gives."""
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
        if not self.on_gpu:
            d, i = self._search(self.X[idx], kk, kstride=ks)
            return d, i, kk, idx, idx
        torch = _torch()
        Xd = self._ds.X
        if isinstance(rows, slice) and rows.indices(N)[2] == 1:
            Qd = Xd[idx[0]:idx[0] + len(idx)] if len(idx) else Xd[:0]  # a view of the device rows
        else:  # a device-to-device gather: no host round trip
            Qd = Xd.index_select(0, torch.from_numpy(idx.astype(np.int64)).to(Xd.device))
        d, i = self._search(Qd, kk, kstride=ks)
        return d, i, kk, idx, torch.from_numpy(idx).to(Xd.device)
