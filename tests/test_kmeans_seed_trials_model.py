"""CPU tier of the greedy seeding: dmlp_cpu_kmeans_seed_trials on one and four threads and
KMeans(seeding="greedy") against tests/helpers/kmeans_seed_trials_contract.py, bit for bit."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.models import KMeans
from distributed_machine_learning_project_amd.ops import knn as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import kmeans_seed_contract as SC  # noqa: E402
import kmeans_seed_trials_contract as TC  # noqa: E402


@pytest.mark.parametrize("case", TC.CASES, ids=str)
def test_trials_twin(case):
    X, i0, u, ref = TC.trials_case(*case)
    for nthreads in (1, 4):
        TC.check(K.kmeans_seed_cpu(X, case[2], i0, u, nthreads=nthreads), ref)
    # what the case is there for
    if case in TC.OLD:
        old = SC.seed_case(*case[:3], case[4])
        for got in (old[3], K.kmeans_seed_cpu(X, case[2], i0, old[2])):     # the 1-D u
            TC.check(got, ref)
    elif case in TC.TIES:
        assert ref[3] > 0                               # a step with equal least potentials
        if case[4] == "equal":
            np.testing.assert_array_equal(ref[0][1:], (u[:, 0] * case[0]).astype(int))
    elif case[4] == "nonfinite":
        assert not {5, 70} & set(ref[0]) and np.isinf(ref[2][[5, 70]]).all()


def test_kmeans_greedy_cpu():
    X, Kc, seed, d2_rows = SC.model_case()
    g = np.random.default_rng(seed)
    i0 = int(g.integers(len(X)))
    rows = TC.ref_seed_trials(X, Kc, 3, i0, g.random((Kc - 1, 3)))[0]   # 2 + int(ln 4) trials
    km = KMeans(Kc, seed, device="cpu", seeding="greedy").fit(X)
    np.testing.assert_array_equal(km.seed_rows_, rows)
    one = KMeans(Kc, seed, device="cpu", seeding="greedy", n_local_trials=1).fit(X)
    np.testing.assert_array_equal(one.seed_rows_, d2_rows)              # one trial: the "d2" draws
    for kw in (dict(n_local_trials=0), dict(n_local_trials=17), dict(n_local_trials=2.5),
               dict(n_local_trials=True), dict(seeding="d2", n_local_trials=3),
               dict(init="first")):
        with pytest.raises(ValueError):
            KMeans(Kc, **{**dict(init=seed, device="cpu", seeding="greedy"), **kw})


def test_trials_arguments_cpu():
    """-1 for what dmlp.h lists, outputs untouched; N = 0 and K = 0 do nothing"""
    X, i0, u, _ = TC.trials_case(65, 33, 9, 4, "int")
    for bad in (dict(u=u[:3]), dict(u=u + 1.0), dict(u=np.zeros((8, 17))), dict(u=np.zeros((8, 0)))):
        with pytest.raises(ValueError):
            K.kmeans_seed_cpu(X, **{**dict(K=9, i0=i0, u=u), **bad})
    seeds, C, w = np.full(9, -5, np.int32), np.full((9, 33), 7.0), np.full(65, 7.0)
    p = [X.ctypes.data, 65, 33, 9, 4, i0, u.ctypes.data, seeds.ctypes.data, C.ctypes.data,
         w.ctypes.data, 1]
    L = _lib.lib()
    for i, bad in ((0, None), (1, 1 << 31), (2, 0), (4, 0), (4, 17), (5, 65), (5, -1), (6, None),
                   (7, None), (8, None), (9, None)):
        assert L.dmlp_cpu_kmeans_seed_trials(*(p[:i] + [bad] + p[i + 1:])) == -1, i
    for i in (1, 3):
        assert L.dmlp_cpu_kmeans_seed_trials(*(p[:i] + [0] + p[i + 1:])) == 0
    assert (seeds == -5).all() and (C == 7.0).all() and (w == 7.0).all()
