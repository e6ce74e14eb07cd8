"""DBSCAN on the engine's distance: density clustering without a neighbour graph in memory.

With d the engine's fp64 squared distance and r2 ONE squared radius (the boundary inclusive):
  core     row i is a core row iff #{n : d(x_i, x_n) <= r2} >= min_samples — the row itself counts,
           as in scikit-learn (one radius count with the rows as their own queries)
  cluster  a connected component of the core rows under d <= r2 (ops.knn.radius_components_*: a
           union-find fed by the distance tile's hits, no CSR); clusters are numbered 0 .. C - 1 in
           ascending order of their smallest core row id, which is scikit-learn's numbering of the
           core samples
  border   a non-core row with a core row within r2 takes the cluster of its NEAREST core row under
           (dist asc, id desc) (an exact search at k = 1) — scikit-learn's border rule depends on
           its traversal order, this one does not
  noise    every other row, label -1
On a GPU the rows go to the device once and only labels_ and the core ids come back.  Both devices
give identical labels.  Not offered yet: sample_weight, and a multi-rank front end.
"""
from __future__ import annotations

import numpy as np

from ..ops import knn as K
from ..ops.knn import _torch
from ._knn_base import squared_radius


class DBSCAN:
    def __init__(self, eps=None, *, r2=None, min_samples: int = 5, device: str = "auto"):
        """Exactly one of eps and r2 (scalars): eps is squared in fp64 once, and a negative or NaN
        eps raises; r2 passes as it is (a negative or NaN one links nothing: every row is noise)."""
        v = squared_radius(eps, r2, "eps")
        if v.ndim:
            raise ValueError("eps / r2 must be a scalar")
        if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or \
                min_samples < 1:
            raise ValueError("min_samples must be an int >= 1")
        self.r2 = float(v)
        self.min_samples = int(min_samples)
        self.on_gpu = device == "gpu" or (device == "auto" and _torch().cuda.is_available())

    # ------------------------------------------------------------ fit
    def fit(self, X):
        X = np.ascontiguousarray(X, np.float64)
        if X.ndim != 2 or X.shape[1] < 1:
            raise ValueError("X must be [N, A] with A >= 1")
        self.labels_, self.core_sample_indices_, self.n_clusters_ = \
            (self._fit_gpu if self.on_gpu else self._fit_cpu)(X)
        return self

    def fit_predict(self, X):
        return self.fit(X).labels_

    def _fit_cpu(self, X):
        N = X.shape[0]
        count = K.radius_count_cpu(X, X, self.r2)
        is_core = count >= self.min_samples
        core = np.flatnonzero(is_core).astype(np.int32)
        # core ids ascend, so ranks in the gathered rows order like row ids: a component's root
        # (its smallest rank) is its smallest core row, and the rank of the root among the roots
        # is the cluster's number
        self._core_rows = X[core]
        comp = K.radius_components_cpu(self._core_rows, self.r2)
        roots, rank = np.unique(comp, return_inverse=True)
        self._core_labels = rank.astype(np.int32).reshape(-1)
        labels = np.full(N, -1, np.int32)
        labels[core] = self._core_labels
        rest = np.flatnonzero(~is_core)
        if len(rest) and len(core):
            labels[rest] = self._nearest_core_cpu(X[rest])
        return labels, core, len(roots)

    def _nearest_core_cpu(self, Q):
        d, i = K.knn_cpu(self._core_rows, Q, np.ones(len(Q), np.int32), kstride=1)
        d, i = d[:, 0], i[:, 0]
        with np.errstate(invalid="ignore"):
            near = (i >= 0) & (d <= self.r2)
        return np.where(near, self._core_labels[np.where(near, i, 0)], -1).astype(np.int32)

    def _fit_gpu(self, X):
        torch = _torch()
        N = X.shape[0]
        Xd = torch.from_numpy(X).cuda()
        count = K.radius_count_gpu(K.prepare_dataset(Xd), Xd, self.r2)
        is_core = count >= self.min_samples
        core = torch.nonzero(is_core).flatten()          # int64, ascending
        self._core_rows = Xd.index_select(0, core)
        comp = K.radius_components_gpu(self._core_rows, self.r2)
        roots = torch.unique(comp)                       # sorted: rank = the cluster's number
        self._core_labels = torch.searchsorted(roots, comp).to(torch.int32)
        labels = torch.full((N,), -1, dtype=torch.int32, device=Xd.device)
        labels[core] = self._core_labels
        rest = torch.nonzero(~is_core).flatten()
        if len(rest) and len(core):
            labels[rest] = self._nearest_core_gpu(Xd, rest.to(torch.int32))[rest]
        return labels.cpu().numpy(), core.to(torch.int32).cpu().numpy(), len(roots)

    def _nearest_core_gpu(self, Qd, qidx):
        """int32 [Q] on the device: the border rule for the rows qidx of Qd, -1 elsewhere"""
        torch = _torch()
        d, i = K.exact_nearest_gpu(self._core_rows, Qd, qidx)
        near = (i >= 0) & (d <= self.r2)
        lab = self._core_labels[torch.where(near, i, torch.zeros_like(i)).long()]
        return torch.where(near, lab, torch.full_like(lab, -1))

    # ------------------------------------------------------------ new points
    def predict(self, Q):
        """int32 [Q]: the border rule applied to new points — the cluster of the nearest core row
        within r2 under (dist asc, id desc), else -1."""
        Q = np.ascontiguousarray(Q, np.float64)
        if Q.ndim != 2 or Q.shape[1] != self._core_rows.shape[1]:
            raise ValueError("Q must be [Q, A]")
        if not len(Q) or not len(self.core_sample_indices_):
            return np.full(len(Q), -1, np.int32)
        if not self.on_gpu:
            return self._nearest_core_cpu(Q)
        torch = _torch()
        Qd = torch.from_numpy(Q).cuda()
        qidx = torch.arange(len(Q), dtype=torch.int32, device=Qd.device)
        return self._nearest_core_gpu(Qd, qidx).cpu().numpy()
