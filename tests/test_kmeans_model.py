"""CPU tier of k-means: the host twins dmlp_cpu_kmeans_assign / dmlp_cpu_cluster_sums and the
estimators on the CPU path against the NumPy reference of tests/helpers/kmeans_contract.py, bit
for bit; KMeans against scikit-learn's Lloyd where it imports."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd.models import KMeans
from distributed_machine_learning_project_amd.ops import knn as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import kmeans_contract as KC  # noqa: E402


@pytest.mark.parametrize("case", KC.ASSIGN, ids=lambda c: "-".join(map(str, c)))
def test_assign_twin(case):
    X, C, prev, label, dmin, ndiff = KC.assign_case(*case)
    for nthreads in (1, 4):
        got = K.kmeans_assign_cpu(X, C, prev, nthreads=nthreads)
        np.testing.assert_array_equal(got[0], label)
        np.testing.assert_array_equal(got[1], dmin)     # (+inf and NaN included)
        assert got[2] == ndiff
    assert K.kmeans_assign_cpu(X, C)[2] is None
    assert label[0] == 0 and dmin[0] == 0               # the three-way tie at d = 0
    if len(X) > 1:
        assert label[len(X) // 2] == 0 and np.isinf(dmin[len(X) // 2])


@pytest.mark.parametrize("A", [1, 33, 65])
@pytest.mark.parametrize("with_extra", [False, True])
def test_cluster_sums_twin(A, with_extra):
    X, label, Kc, extra = KC.sums_case(A)
    extra = extra if with_extra else None
    ref = KC.ref_sums(X, label, Kc, extra)
    # the case proves something: the ordered sum is not what np.sum gives for the same members
    assert (ref[5, :A] != X[label == 5].sum(axis=0)).any()
    C = np.full((Kc, A), 7.0)
    sums, count = K.cluster_sums_cpu(X, label, Kc, extra, centroids=C, nthreads=4)
    np.testing.assert_array_equal(KC.bits(sums), KC.bits(ref))
    np.testing.assert_array_equal(count, [0, 1, 63, 64, 65, 129])
    np.testing.assert_array_equal(KC.bits(C[1:]), KC.bits(ref[1:, :A] / count[1:, None]))
    assert (C[0] == 7.0).all()                          # the empty cluster keeps its centroid


@pytest.mark.parametrize("fit", KC.FITS, ids=lambda f: f[0])
def test_kmeans_cpu(fit):
    X, init, tol, _, _ = KC.fit_case(fit[0])
    KC.check_fit(KMeans(fit[2], init, tol=tol, device="cpu").fit(X), fit[0])


def test_kmeans_arguments():
    X = KC.fit_case("first")[0]
    for kw in (dict(n_clusters=0, init="first"), dict(n_clusters=3, init="first", max_iter=0),
               dict(n_clusters=3, init="first", tol=-1.0)):
        with pytest.raises(ValueError):
            KMeans(device="cpu", **kw)
    for init in ("k-means++", np.zeros((2, 2)), np.zeros((3, 5))):
        with pytest.raises(ValueError):
            KMeans(3, init, device="cpu").fit(X)
    with pytest.raises(ValueError):
        KMeans(300, "first", device="cpu").fit(X)
    with pytest.raises(ValueError):
        K.cluster_sums_cpu(X, np.full(len(X), 3, np.int32), 3)


def test_nearest_centroid_cpu():
    KC.check_nearest_centroid("cpu")


def test_sklearn_lloyd():
    cluster = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(0)
    X = rng.normal(0, 1, (300, 4)) + 20 * rng.integers(0, 3, (300, 1))
    C0 = X[[np.flatnonzero(X[:, 0].round(-1) == v)[0] for v in (0, 20, 40)]]
    km = KMeans(3, C0, device="cpu").fit(X)
    sk = cluster.KMeans(3, init=C0, n_init=1, algorithm="lloyd").fit(X)
    np.testing.assert_array_equal(km.labels_, sk.labels_)
    assert np.allclose(km.cluster_centers_, sk.cluster_centers_)
