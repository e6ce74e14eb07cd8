"""KMeans (Lloyd) and NearestCentroid on the engine's distance, bit-identical on both devices.

Two ops carry both estimators (ops.knn, csrc/kmeans.hip, dmlp.h "k-means"):
  assign   label[i] = the SMALLEST c minimising d(x_i, C_c), d the engine's fp64 squared distance;
           a NaN distance ranks as +inf, a row without a finite distance takes label 0
  sums     per-cluster sums of the member rows in a FIXED order: members in ascending row id, cut
           into runs of 64, a run summed left to right, the run sums added left to right — no
           floating-point atomics, so the result does not change from run to run
Lloyd step: centroid c = sums[c] / count[c] (IEEE division); an empty cluster keeps its centroid.
The fit stops when an assignment changes no label, when the squared centroid shift — summed on the
host over the K x A centroids in row-major order — is <= tol (tol > 0 only), or at max_iter.  Both
devices hold identical centroids, so both stop at the same iteration.  labels_ and inertia_ always
belong to cluster_centers_: inertia_ is the left-to-right sum over the clusters of the ordered sums
of the members' distances.  On a GPU the rows go to the device once; per iteration only the
changed count and, for tol > 0, the K x A centroids come back.

assign= chooses the GPU's way to the assignment, never its result: "exact" is the fp64 tile over
all K centroids, "screen" the bf16 MFMA screen with an exact re-rank of its few candidates
(csrc/kmeans_screen.hip; the row operands are made once per fit), "auto" the screen from
K >= kAssignScreenK on.  A > 128 and the CPU always take the exact way.

seeding="d2" with init=<int seed> is k-means++ seeding (ops.knn.kmeans_seed_*, csrc/kmeans_seed.hip,
dmlp.h "k-means seeding"): the first seed is row i0, each further one the row at which the running
sum of the rows' distances to their nearest seed so far passes u times its total.  The sums run in
a fixed order (runs of 64 rows, blocks of 64 runs, the blocks left to right), so both devices pick
the same rows; the draws come from the host: rng = numpy.random.default_rng(seed), i0 =
int(rng.integers(N)), u = rng.random(K - 1).  On a GPU the rows go over first and the K seeds are
picked there without a host sync.  The spelling is a keyword of its own because the string init
"k-means++" has always been a ValueError here and stays one; seeding="uniform" (the default) is
the draw of K distinct rows, as before.

seeding="greedy" is greedy k-means++ (dmlp.h "k-means seeding, local trials"): every step draws
L = n_local_trials candidates that way (None: 2 + int(ln K); an int in 1 .. 16) and keeps the one
that leaves the least sum of the rows' distances to their nearest seed, the first of equals.  The
draws: rng as above, i0 = int(rng.integers(N)), u = rng.random((K - 1, L)); with L = 1 this is
"d2", draw for draw and bit for bit.  On a GPU one pass over X per step serves all L trials
(k_seed_trial, csrc/kmeans_seed.hip), again without a host sync.

Not offered yet: n_init restarts, sample_weight, a multi-rank
front end, a 3-term (hi/lo) screen for tightly packed centroids, the screen at A > 128.
"""
from __future__ import annotations

import numpy as np

from ..ops import knn as K
from ..ops.knn import _torch


def _sum_lr(v) -> float:
    """((v_0 + v_1) + v_2) ...: np.add.accumulate is the sequential sum, np.sum is pairwise"""
    v = np.asarray(v, np.float64).ravel()
    return float(np.add.accumulate(v)[-1]) if v.size else 0.0


# assign="auto" screens from this K on: the smallest measured K from which the screened assignment
# is ahead of the exact one by more than the spread of both at every larger measured K
# (profiles/kmeans_screen.md: ahead at K = 256, 1024 and 4096 for N = 1e5 and 1e6, A = 32 and 128;
# at K = 64 behind at A = 128; nothing in between was measured)
kAssignScreenK = 256
kScreenMaxA = 128


class _Ops:
    """assign / sums on host arrays or on one GPU, behind the same calls"""

    def __init__(self, device: str, assign: str = "auto"):
        if assign not in ("exact", "screen", "auto"):
            raise ValueError('assign must be "exact", "screen" or "auto"')
        self.on_gpu = device == "gpu" or (device == "auto" and _torch().cuda.is_available())
        self.mode = assign
        self.sums = K.cluster_sums_gpu if self.on_gpu else K.cluster_sums_cpu

    def rows(self, Xd, Kc: int):
        """what assign takes for these rows against Kc centroids: the rows themselves, or — where
        the choice is the screen — its row operands around them, made here once"""
        screen = self.on_gpu and Xd.shape[1] <= kScreenMaxA and (
            self.mode == "screen" or
            (self.mode == "auto" and kAssignScreenK is not None and Kc >= kAssignScreenK))
        return K.kmeans_rows_gpu(Xd) if screen else Xd

    def assign(self, Xr, C, prev=None):
        if not self.on_gpu:
            return K.kmeans_assign_cpu(Xr, C, prev)
        return K.kmeans_assign_gpu(Xr, C, prev, screen=isinstance(Xr, K.KMeansRows))

    def put(self, a):
        return _torch().from_numpy(np.ascontiguousarray(a)).cuda() if self.on_gpu else a

    def get(self, t):
        return t.cpu().numpy() if self.on_gpu else t


def _rows(X, name: str = "X", A=None):
    X = np.ascontiguousarray(X, np.float64)
    if X.ndim != 2 or X.shape[1] < 1 or (A is not None and X.shape[1] != A):
        raise ValueError(f"{name} must be [N, A]" + (" with A >= 1" if A is None else ""))
    return X


class KMeans:
    def __init__(self, n_clusters: int, init, max_iter: int = 300, tol: float = 0.0,
                 device: str = "auto", assign: str = "auto", seeding: str = "uniform",
                 n_local_trials=None):
        """init: a [K, A] array of centroids, "first" (rows 0 .. K - 1 of X), or an int seed (K
        distinct rows of X drawn by numpy.random.default_rng(seed).choice, taken in ascending row
        id).  seeding="d2", with an int seed only: D^2 (k-means++) seeding from that generator;
        seed_rows_ then holds the K seed rows.  seeding="greedy", likewise: n_local_trials
        candidates per step (None: 2 + int(ln K); else an int in 1 .. 16), the best one kept."""
        for v, name in ((n_clusters, "n_clusters"), (max_iter, "max_iter")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be an int >= 1")
        if not float(tol) >= 0.0:
            raise ValueError("tol must be >= 0")
        self.n_clusters, self.max_iter, self.tol = int(n_clusters), int(max_iter), float(tol)
        if seeding not in ("uniform", "d2", "greedy"):
            raise ValueError('seeding must be "uniform", "d2" or "greedy"')
        if seeding != "uniform" and not self._is_seed(init):
            raise ValueError(f'seeding="{seeding}" needs init=<int seed>')
        if n_local_trials is not None and (seeding != "greedy" or not self._is_seed(n_local_trials)
                                           or not 1 <= n_local_trials <= 16):
            raise ValueError('n_local_trials: an int in 1 .. 16, with seeding="greedy" only')
        if seeding == "greedy":
            # None: scikit-learn's count, within 1 .. 16 for any K an int32 holds
            self.n_local_trials = int(n_local_trials) if n_local_trials is not None else \
                2 + int(np.log(self.n_clusters))
        self.init, self.seeding = init, seeding
        self._ops = _Ops(device, assign)
        self.on_gpu = self._ops.on_gpu

    @staticmethod
    def _is_seed(init) -> bool:
        return isinstance(init, (int, np.integer)) and not isinstance(init, bool)

    def _seed_d2(self, Xd):
        """(seeds, C) where Xd lies: the D^2 seeding of the rows from init's generator, greedy
        with a 2-D u"""
        N, Kc = Xd.shape[0], self.n_clusters
        if N < Kc:
            raise ValueError(f"{N} rows cannot seed {Kc} clusters")
        rng = np.random.default_rng(int(self.init))
        i0 = int(rng.integers(N))
        u = rng.random(Kc - 1 if self.seeding == "d2" else (Kc - 1, self.n_local_trials))
        seed = K.kmeans_seed_gpu if self.on_gpu else K.kmeans_seed_cpu
        return seed(Xd, Kc, i0, u)[:2]

    def _init_centroids(self, X):
        Kc, init = self.n_clusters, self.init
        seed = self._is_seed(init)
        if isinstance(init, str) and init != "first":
            raise ValueError('init must be a [K, A] array, "first" or an int seed')
        if isinstance(init, str) or seed:
            if X.shape[0] < Kc:
                raise ValueError(f"{X.shape[0]} rows cannot seed {Kc} clusters")
            rows = np.sort(np.random.default_rng(int(init)).choice(X.shape[0], Kc, replace=False)) \
                if seed else np.arange(Kc)
            return X[rows].copy()
        C0 = np.array(init, np.float64, order="C")
        if C0.shape != (Kc, X.shape[1]):
            raise ValueError("an init array must be [n_clusters, A]")
        return C0

    def fit(self, X):
        X = _rows(X)
        if not X.shape[0]:
            raise ValueError("X has no rows")
        o, Kc, A = self._ops, self.n_clusters, X.shape[1]
        if self.seeding != "uniform":
            Xd = o.put(X)                   # the rows go over first: the seeds are picked there
            seeds, C = self._seed_d2(Xd)    # C is updated in place by the Lloyd step
            self.seed_rows_ = o.get(seeds)
            Ch = o.get(C).copy()            # the host's copy: the shift's "before"
        else:
            Ch = self._init_centroids(X)
            Xd, C = o.put(X), o.put(Ch.copy())
        Xr = o.rows(Xd, Kc)
        prev, fresh, self.n_iter_ = None, False, 0
        for it in range(self.max_iter):
            label, dmin, changed = o.assign(Xr, C, prev)
            if prev is not None and int(changed) == 0:
                fresh = True                # label and dmin belong to C
                break
            o.sums(Xd, label, Kc, centroids=C)
            self.n_iter_, prev = it + 1, label
            if self.tol > 0.0:
                Cn = o.get(C).copy()
                diff = (Cn - Ch).ravel()
                Ch = Cn
                if _sum_lr(diff * diff) <= self.tol:
                    break
        if not fresh:
            label, dmin, _ = o.assign(Xr, C)
        sums, _ = o.sums(Xd, label, Kc, extra=dmin)
        self.cluster_centers_ = o.get(C).copy()
        self.labels_ = o.get(label)
        self.inertia_ = _sum_lr(o.get(sums[:, A]))
        return self

    def fit_predict(self, X):
        return self.fit(X).labels_

    def predict(self, Q):
        """int32 [Q]: the nearest centroid of each row, ties to the smaller cluster"""
        Q = _rows(Q, "Q", self.cluster_centers_.shape[1])
        o = self._ops
        Qr = o.rows(o.put(Q), self.n_clusters)
        return o.get(o.assign(Qr, o.put(self.cluster_centers_))[0])


class NearestCentroid:
    """The nearest-centroid classifier: centroids_ are the ORDERED class means (the ordered sums
    of each class's rows over its count), predict the class of the nearest centroid.  A tie goes
    to the SMALLER class — the assignment's rule, unlike the k-NN vote (larger label)."""

    def __init__(self, device: str = "auto", assign: str = "auto"):
        self._ops = _Ops(device, assign)
        self.on_gpu = self._ops.on_gpu

    def fit(self, X, y):
        X = _rows(X)
        y = np.asarray(y)
        if y.shape != (X.shape[0],) or not X.shape[0]:
            raise ValueError("y must be [N], N >= 1")
        o = self._ops
        self.classes_, rank = np.unique(y, return_inverse=True)
        C = o.put(np.zeros((len(self.classes_), X.shape[1]), np.float64))
        o.sums(o.put(X), o.put(rank.reshape(-1).astype(np.int32)), len(self.classes_), centroids=C)
        self.centroids_ = o.get(C).copy()
        return self

    def predict(self, Q):
        Q = _rows(Q, "Q", self.centroids_.shape[1])
        o = self._ops
        Qr = o.rows(o.put(Q), len(self.classes_))
        return self.classes_[o.get(o.assign(Qr, o.put(self.centroids_))[0])]
