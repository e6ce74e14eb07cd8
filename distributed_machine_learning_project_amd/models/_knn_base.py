"""What the k-NN estimators share: the fitted rows on the host and, on a GPU, on the device; Update
records; the exact search (ops.knn.knn_gpu without the fused vote on a GPU, knn_cpu otherwise); the
radius search (radius_count, radius_neighbors, and the padded lists behind the estimators'
radius_predict); and the front of every leave-one-out call, which turns dataset rows into queries
against the dataset itself.  An estimator adds fit(), a one-line _prepare() and the kernels that read the sorted lists
(votes for KNNClassifier, neighbour means for KNNRegressor).
"""
from __future__ import annotations

import numpy as np

from ..ops import knn as K
from ..ops.knn import _torch


def squared_radius(radius, r2, name: str = "radius"):
    """The squared radius (float64, shaped like the argument) of a call that takes exactly one of a
    radius and r2.  radius: r2 = radius * radius in fp64 (one rounding); negative or NaN raises.
    r2 passes as it is: a negative or NaN one keeps nothing."""
    if (radius is None) == (r2 is None):
        raise ValueError(f"give exactly one of {name} and r2")
    v = np.asarray(radius if r2 is None else r2, np.float64)
    if r2 is None:
        if np.isnan(v).any() or (v < 0).any():
            raise ValueError(f"{name} must be >= 0")
        with np.errstate(over="ignore"):
            v = v * v
    return v


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

    # ------------------------------------------------------------ radius search
    # Every point within a radius instead of the k nearest (csrc/radius.hip; dmlp_cpu_radius_* on a
    # CPU): one count launch over all queries, then fill + sort in contiguous batches of queries.
    # A query's neighbours under (dist asc, id desc) are the first count_q entries of its k-NN
    # list, so every radius result equals the k-NN one at the per-query k = count.
    def _radius_r2(self, Q, radius, r2):
        """The squared radii float64 [Q] of a radius call: exactly one of radius and r2, a scalar
        or [Q].  radius: r2 = radius * radius in fp64 (one rounding); negative or NaN raises.  r2
        passes as it is: a negative or NaN one keeps nothing."""
        v = squared_radius(radius, r2)
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != Q.shape[0]):
            raise ValueError("radius / r2 must be a scalar or [Q]")
        return np.ascontiguousarray(np.broadcast_to(v, (Q.shape[0],)))

    def _radius_front(self, Q, radius, r2):
        """(queries, squared radii, counts) of a radius call — on the device for a GPU — and the
        counts on the host."""
        Q = np.ascontiguousarray(Q, np.float64)
        if Q.ndim != 2 or Q.shape[1] != self.X.shape[1]:
            raise ValueError("Q must be [Q, A]")
        rr = self._radius_r2(Q, radius, r2)
        if self.on_gpu:
            torch = _torch()
            Qd, rd = torch.from_numpy(Q).cuda(), torch.from_numpy(rr).cuda()
            cd = K.radius_count_gpu(self._ds, Qd, rd)
            return Qd, rd, cd, cd.cpu().numpy()
        c = K.radius_count_cpu(self.X, Q, rr)
        return Q, rr, c, c

    @staticmethod
    def _radius_batches(count, max_entries, padded):
        """Contiguous query ranges [a, b) whose entries stay at or below max_entries — the sum of
        the counts (CSR), or rows x the largest count (padded lists); a single query larger than
        that is a range of its own."""
        max_entries = max(1, int(max_entries))
        a, n = 0, len(count)
        while a < n:
            b, tot, cmax = a, 0, 0
            while b < n:
                c = int(count[b])
                size = (b + 1 - a) * max(cmax, c) if padded else tot + c
                if b > a and size > max_entries:
                    break
                tot, cmax, b = tot + c, max(cmax, c), b + 1
            yield a, b
            a = b

    def _radius_search(self, Qx, rr, cnt, a, b, sort=True, stride=None):
        if self.on_gpu:
            return K.radius_gpu(self._ds, Qx[a:b], rr[a:b], sort=sort, stride=stride, count=cnt[a:b])
        return K.radius_cpu(self.X, Qx[a:b], rr[a:b], sort=sort, stride=stride, count=cnt[a:b])

    def radius_count(self, Q, radius=None, *, r2=None):
        """int32 [Q]: the fitted rows within `radius` of each query — or within the SQUARED radius
        `r2`; exactly one of the two, a scalar or a [Q] array.  The test is dist <= r2 on the
        engine's squared distances, boundary included; radius is squared in fp64 first (one
        rounding), so pass r2 where the boundary matters to the bit."""
        return self._radius_front(Q, radius, r2)[3]

    def radius_neighbors(self, Q, radius=None, *, r2=None, sort_results: bool = True,
                         max_entries: int = 2 ** 26):
        """(indptr int64 [Q + 1], dist float64 [total], ids int32 [total]) in CSR: query q's
        neighbours are slots [indptr[q], indptr[q + 1]), ordered by (dist asc, id desc) — the head
        of kneighbors' list — or by descending id with sort_results=False.  The queries are worked
        in contiguous batches of at most max_entries entries (a larger single query is a batch of
        its own).  Bit-identical on both devices."""
        Qx, rr, cnt, count = self._radius_front(Q, radius, r2)
        indptr = np.zeros(len(count) + 1, np.int64)
        np.cumsum(count, out=indptr[1:])
        d = np.empty(int(indptr[-1]), np.float64)
        i = np.empty(int(indptr[-1]), np.int32)
        for a, b in self._radius_batches(count, max_entries, padded=False):
            _, bd, bi = self._radius_search(Qx, rr, cnt, a, b, sort=sort_results)
            d[indptr[a]:indptr[b]] = self._host(bd)
            i[indptr[a]:indptr[b]] = self._host(bi)
        return indptr, d, i

    def _radius_lists(self, Q, radius, r2, max_entries):
        """The sorted neighbours as padded lists, batch by batch: (a, b, dist [b - a, s], ids, count
        [b - a]) with s the batch's largest count (at least 1) and (b - a) s <= max_entries; on the
        device for a GPU.  The list kernels read them with k = count."""
        Qx, rr, cnt, count = self._radius_front(Q, radius, r2)
        for a, b in self._radius_batches(count, max_entries, padded=True):
            s = max(1, int(count[a:b].max()))
            d, i, c = self._radius_search(Qx, rr, cnt, a, b, stride=s)
            yield a, b, d, i, c

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
