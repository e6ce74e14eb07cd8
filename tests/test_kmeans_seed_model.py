"""CPU tier of the D^2 seeding: the host twin dmlp_cpu_kmeans_seed on one and four threads and
KMeans(seeding="d2") on the CPU path against the NumPy reference of
tests/helpers/kmeans_seed_contract.py, bit for bit."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.models import KMeans
from distributed_machine_learning_project_amd.ops import knn as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import kmeans_seed_contract as SC  # noqa: E402


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: "-".join(map(str, c)))
def test_seed_twin(case):
    X, i0, u, (seeds, _, w) = SC.seed_case(*case)
    for nthreads in (1, 4):
        SC.check(K.kmeans_seed_cpu(X, case[2], i0, u, nthreads=nthreads), case)
    # what the case is there for
    if case[3] == "nonfinite":
        assert not {5, 70} & set(seeds) and np.isinf(w[[5, 70]]).all()
    elif case[3] == "equal":
        np.testing.assert_array_equal(seeds[1:], (u * case[0]).astype(int))
    elif case[3] == "absorb":
        assert seeds[1] == SC.ABSORB_PICK[case[0]]
    elif case[3] == "gauss":
        assert len(set(seeds)) == case[2] and (w[seeds] == 0).all()
    elif case[0] > 1:
        assert (w == 0).sum() > len(set(seeds))         # the seeds' copies


def test_kmeans_d2_cpu():
    X, Kc, seed, rows = SC.model_case()
    km = KMeans(Kc, seed, device="cpu", seeding="d2").fit(X)
    np.testing.assert_array_equal(km.seed_rows_, rows)
    assert km.seed_rows_.dtype == np.int32 and km.n_iter_ >= 1
    ref = KMeans(Kc, X[rows], device="cpu").fit(X)      # the same Lloyd run from those rows
    np.testing.assert_array_equal(SC.bits(km.cluster_centers_), SC.bits(ref.cluster_centers_))
    assert (km.n_iter_, km.inertia_) == (ref.n_iter_, ref.inertia_)
    for kw in (dict(init="first", seeding="d2"), dict(init=X[:Kc], seeding="d2"),
               dict(init=seed, seeding="k-means++")):
        with pytest.raises(ValueError):
            KMeans(Kc, device="cpu", **kw).fit(X)
    with pytest.raises(ValueError):
        KMeans(301, seed, device="cpu", seeding="d2").fit(X)


def test_seed_arguments_cpu():
    """-1 for what dmlp.h lists, outputs untouched; N = 0 and K = 0 do nothing"""
    X, i0, u, _ = SC.seed_case(65, 33, 9, "int")
    for bad in (dict(K=0), dict(i0=65), dict(i0=-1), dict(u=u[:3]), dict(u=u + 1.0)):
        with pytest.raises(ValueError):
            K.kmeans_seed_cpu(X, **{**dict(K=9, i0=i0, u=u), **bad})
    seeds, C, w = np.full(9, -5, np.int32), np.full((9, 33), 7.0), np.full(65, 7.0)
    p = [X.ctypes.data, 65, 33, 9, i0, u.ctypes.data, seeds.ctypes.data, C.ctypes.data,
         w.ctypes.data, 1]
    L = _lib.lib()
    for i, bad in ((0, None), (1, 1 << 31), (2, 0), (4, 65), (4, -1), (5, None), (6, None),
                   (7, None), (8, None)):
        assert L.dmlp_cpu_kmeans_seed(*(p[:i] + [bad] + p[i + 1:])) == -1, i
    for i in (1, 3):
        assert L.dmlp_cpu_kmeans_seed(*(p[:i] + [0] + p[i + 1:])) == 0
    assert (seeds == -5).all() and (C == 7.0).all() and (w == 7.0).all()
