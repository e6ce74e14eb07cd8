"""Plain NumPy reference of the k-means ops (dmlp.h "k-means") and the cases the CPU and GPU
tests share: distances by ops/reference.py, argmin with the tie rule (np.argmin: the first, i.e.
smallest, index; NaN ranked as +inf), Python loops for the run-of-64 sums and the Lloyd loop."""
import functools

import numpy as np

from distributed_machine_learning_project_amd.models import NearestCentroid
from distributed_machine_learning_project_amd.ops import reference as R

INF = np.inf
# (N, A, K): the 64-row workgroup, the 16-attribute chunk and its odd tail, both tile widths (16
# and 128 centroids), their pad columns and a second tile
ASSIGN = [(1, 1, 1), (63, 15, 15), (65, 17, 16), (130, 33, 17), (130, 16, 129), (65, 1, 129)]


def ref_assign(X, C):
    label, dmin = np.zeros(len(X), np.int32), np.zeros(len(X))
    for i, x in enumerate(X):
        with np.errstate(invalid="ignore"):
            d = R.distances(C, x)
        label[i] = np.argmin(np.where(np.isnan(d), INF, d))
        dmin[i] = d[label[i]]
    return label, dmin


def ref_sums(X, label, K, extra=None):
    V = X if extra is None else np.column_stack([X, extra])
    sums = np.zeros((K, V.shape[1]))
    for c in range(K):
        m = np.flatnonzero(label == c)
        for r0 in range(0, len(m), 64):
            run = np.zeros(V.shape[1])
            for i in m[r0:r0 + 64]:
                run = run + V[i]
            sums[c] = sums[c] + run
    return sums


def sum_lr(v):
    s = 0.0
    for x in np.asarray(v).ravel():
        s = s + float(x)
    return s


@functools.lru_cache(maxsize=None)
def assign_case(N, A, K):
    """(X, C, prev, label, dmin, ndiff): duplicate centroids (0, K // 2, K - 1), row 0 equal to
    them (d = 0, a three-way tie), a centroid holding +inf (NaN against the +inf row), one row
    holding +inf (no finite distance: label 0), prev differing from label in ndiff rows"""
    rng = np.random.default_rng(1000 * N + 10 * A + K)
    X, C = np.round(rng.uniform(-4, 4, (N, A)), 3), np.round(rng.uniform(-4, 4, (K, A)), 3)
    C[K // 2] = C[K - 1] = C[0]
    if K >= 15:
        C[1, 0] = INF
    X[0] = C[0]
    if N > 1:
        X[N // 2, 0] = INF
    label, dmin = ref_assign(X, C)
    prev = label.copy()
    prev[::3] += 1
    return X, C, prev, label, dmin, len(prev[::3])


@functools.lru_cache(maxsize=None)
def sums_case(A):
    """(X, label, K, extra): cluster sizes {0, 1, 63, 64, 65, 129} in shuffled rows; values over
    many binades, so that the order of a sum changes its bits"""
    sizes = [0, 1, 63, 64, 65, 129]
    rng = np.random.default_rng(A)
    label = rng.permutation(np.repeat(np.arange(6), sizes)).astype(np.int32)
    vals = np.array([1e16, 1.0, -1e16, 3.0, 0.5])
    return rng.choice(vals, (len(label), A)), label, 6, rng.choice(vals, len(label))


def ref_lloyd(X, C0, max_iter, tol):
    """(centers, labels, inertia, n_iter) of models/kmeans.py's loop over the reference ops"""
    C, K, prev, fresh, n_iter = C0.copy(), len(C0), None, False, 0
    for it in range(max_iter):
        label, dmin = ref_assign(X, C)
        if prev is not None and (label == prev).all():
            fresh = True
            break
        sums, count = ref_sums(X, label, K), np.bincount(label, minlength=K)
        Cn = C.copy()
        Cn[count > 0] = sums[count > 0] / count[count > 0, None]
        shift, C, n_iter, prev = sum_lr((Cn - C) ** 2), Cn, it + 1, label
        if tol > 0 and shift <= tol:
            break
    if not fresh:
        label, dmin = ref_assign(X, C)
    return C, label, sum_lr(ref_sums(dmin[:, None], label, K)[:, 0]), n_iter


# (name, A, K, init, tol): "empty" starts with a centroid no row is nearest to
FITS = [("first", 2, 3, "first", 0.0), ("seed", 17, 17, 5, 1e-3), ("empty", 2, 3, None, 0.0)]


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """(X, init, tol, held-out Q, ref_lloyd's result): 200 rows in three blobs"""
    _, A, K, init, tol = next(f for f in FITS if f[0] == name)
    rng = np.random.default_rng(A)
    X = np.round(rng.normal(0, 1, (200, A)) + 6 * rng.integers(0, 3, (200, 1)), 3)
    Q = np.round(rng.normal(0, 1, (40, A)) + 6 * rng.integers(0, 3, (40, 1)), 3)
    if init is None:
        init = np.array([[0.0, 0.0], [12.0, 12.0], [1e3, 1e3]])
    C0 = X[:K] if isinstance(init, str) else init if isinstance(init, np.ndarray) else \
        X[np.sort(np.random.default_rng(init).choice(200, K, replace=False))]
    return X, init, tol, Q, ref_lloyd(X, np.array(C0, np.float64), 300, tol)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def check_fit(km, name):
    """km fitted on fit_case(name): the NumPy Lloyd loop's bits, and predict on held-out rows"""
    X, _, _, Q, (C, label, inertia, n_iter) = fit_case(name)
    np.testing.assert_array_equal(bits(km.cluster_centers_), bits(C))
    np.testing.assert_array_equal(km.labels_, label)
    assert bits(km.inertia_) == bits(inertia) and km.n_iter_ == n_iter and n_iter > 1
    np.testing.assert_array_equal(km.predict(Q), ref_assign(Q, C)[0])


def check_nearest_centroid(device):
    """non-contiguous class labels: the ordered class means, predict mapped through classes_"""
    X, label, _, _ = sums_case(33)
    y = np.array([-7, 2, 40, 41, 90, 1000])[label]        # (class -7 has no member)
    nc = NearestCentroid(device=device).fit(X, y)
    np.testing.assert_array_equal(nc.classes_, [2, 40, 41, 90, 1000])
    ref = ref_sums(X, label, 6)[1:] / np.bincount(label)[1:, None]
    np.testing.assert_array_equal(bits(nc.centroids_), bits(ref))
    Q = np.concatenate([X[:50], (ref[1:2] + ref[3:4]) / 2])
    np.testing.assert_array_equal(nc.predict(Q), nc.classes_[ref_assign(Q, ref)[0]])
