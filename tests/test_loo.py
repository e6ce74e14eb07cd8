"""Choosing k on KNNClassifier: predict_curve, loo_kneighbors, loo_curve, select_k — the CPU path
here, the same cases on the GPU path (the vote-curve kernel behind the native search) under
`gpu`.  The oracle is ops/reference.py's NumPy brute force with the row deleted from the dataset
(ids remapped) and the dict vote of tests/helpers/result_contract.py on its prefixes, so nothing
the leave-one-out plumbing does — the search at kmax + 1, the skip of
the row's own id — is shared with it.  All comparisons are bit-exact."""
import functools
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd.models import KNNClassifier
from distributed_machine_learning_project_amd.ops import reference as ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import result_contract as RC  # noqa: E402

DEVICES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]


@functools.lru_cache(maxsize=None)
def dataset(name):
    """(X, y, kmax).  "triples": N = 600, A = 5, 7 labels, every row three times (each row has two
    neighbours at distance 0, labelled independently); "block": 30 identical rows among 200 — with
    kmax = 8 the search at k = 9 returns the 9 largest ids of the block, so 21 rows are absent from
    their own lists; "tiny": N = 5 < kmax."""
    rng = np.random.default_rng({"triples": 1, "block": 2, "tiny": 3}[name])
    if name == "triples":
        base = np.round(rng.uniform(0, 10, (200, 5)), 3)
        X = np.concatenate([base, base, base])[rng.permutation(600)]
        y = rng.integers(0, 7, 600)
        kmax = 20
    elif name == "block":
        X = np.round(rng.uniform(0, 10, (230, 5)), 3)
        X[100:130] = X[100]
        y = rng.integers(0, 4, 230)
        kmax = 8
    else:
        X = np.round(rng.uniform(0, 10, (5, 5)), 3)
        y = np.array([2, 0, 2, 1, 0])
        kmax = 8
    return np.ascontiguousarray(X), y.astype(np.int32), kmax


@functools.lru_cache(maxsize=None)
def loo_ref(name):
    """(dist [N, kmax], ids [N, kmax], hits [kmax]) by brute force on the dataset without row r."""
    X, y, kmax = dataset(name)
    N = len(X)
    D = np.full((N, kmax), np.inf)
    I = np.full((N, kmax), -1, np.int32)
    hits = np.zeros(kmax, np.int64)
    for r in range(N):
        d, i = ref.topk(np.delete(X, r, axis=0), X[r], kmax)
        i = np.where(i >= r, i + 1, i)
        D[r, :len(i)], I[r, :len(i)] = d, i
        for k in range(1, kmax + 1):
            hits[k - 1] += RC.vote_ref(i, min(k, len(i)), y) == y[r]
    for a in (D, I, hits):
        a.setflags(write=False)
    return D, I, hits


def _fit(device, name, **kw):
    X, y, kmax = dataset(name)
    return KNNClassifier(device=device, **kw).fit(X, y), kmax


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", ["triples", "block", "tiny"])
def test_loo_kneighbors_matches_brute_force(device, name):
    clf, kmax = _fit(device, name)
    D, I, _ = loo_ref(name)
    d, i = clf.loo_kneighbors(kmax)
    assert d.shape == i.shape == (len(I), kmax) and i.dtype == np.int32
    np.testing.assert_array_equal(i, I)
    np.testing.assert_array_equal(d, D)
    assert (i != np.arange(len(I))[:, None]).all()
    # rows: an index array (negative ids count from the end) and a slice
    N = len(I)
    rows = np.array([N - 1, 0, 3, -2, 3])
    d, i = clf.loo_kneighbors(kmax, rows=rows)
    np.testing.assert_array_equal(i, I[rows])
    np.testing.assert_array_equal(d, D[rows])
    d, i = clf.loo_kneighbors(kmax, rows=slice(1, 4))
    np.testing.assert_array_equal(i, I[1:4])
    d, i = clf.loo_kneighbors(3, rows=slice(0, N, 2))
    np.testing.assert_array_equal(i, I[::2, :3])
    np.testing.assert_array_equal(d, D[::2, :3])


@pytest.mark.parametrize("device", DEVICES)
def test_block_rows_are_absent_from_their_own_lists(device):
    """What makes "block" the self-absent case: the search at kmax + 1 does not return the row."""
    clf, kmax = _fit(device, "block")
    X, _, _ = dataset("block")
    _, i = clf.kneighbors(X[100:130], kmax + 1)
    absent = [(r not in i[r - 100]) for r in range(100, 130)]
    assert sum(absent) == 30 - (kmax + 1)


@pytest.mark.parametrize("device", DEVICES)
def test_predict_curve_columns_are_predict(device):
    clf, _ = _fit(device, "triples")
    Q = np.round(np.random.default_rng(7).uniform(0, 10, (130, 5)), 3)
    curve = clf.predict_curve(Q, 20)
    assert curve.shape == (130, 20) and curve.dtype == np.int32
    for k in range(1, 21):
        np.testing.assert_array_equal(curve[:, k - 1], clf.predict(Q, k), err_msg=f"k={k}")
    # more columns than points: the vote of all of them repeats
    tiny, _ = _fit(device, "tiny")
    c = tiny.predict_curve(Q[:9], 8)
    for k in range(1, 9):
        np.testing.assert_array_equal(c[:, k - 1], tiny.predict(Q[:9], k), err_msg=f"tiny k={k}")
    with pytest.raises(ValueError):
        clf.predict_curve(Q, 257)
    with pytest.raises(ValueError):
        clf.predict_curve(Q, 0)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("name", ["triples", "block", "tiny"])
def test_loo_curve_batches_agree(device, name):
    clf, kmax = _fit(device, name)
    _, _, H = loo_ref(name)
    h64, n64 = clf.loo_curve(kmax, batch_rows=64)
    hall, nall = clf.loo_curve(kmax, batch_rows=10 ** 6)
    assert n64 == nall == len(dataset(name)[0])
    assert h64.dtype == np.int64 and h64.shape == (kmax,)
    np.testing.assert_array_equal(h64, hall)
    np.testing.assert_array_equal(h64, H)
    with pytest.raises(ValueError):
        clf.loo_curve(256)


@functools.lru_cache(maxsize=None)
def tie_dataset():
    """Six far-apart clusters of five points on a line: label a = 10 + c at 0, 1, 2, 3 and the
    smaller label b = c at 1.5.  k = 1 misleads the points at 1 and 2 (their nearest is b); from
    k = 2 on the count ties go to the larger label a, so 4 of 5 rows are right for k = 2, 3, 4 and
    the maximum is shared."""
    X, y = [], []
    for c in range(6):
        for x, lab in ((0.0, 10 + c), (1.0, 10 + c), (2.0, 10 + c), (3.0, 10 + c), (1.5, c)):
            X.append([100.0 * c + x, 0.0])
            y.append(lab)
    return np.array(X), np.array(y, np.int32)


@pytest.mark.parametrize("device", DEVICES)
def test_select_k_takes_the_smallest_best_k(device):
    X, y = tie_dataset()
    clf = KNNClassifier(device=device).fit(X, y)
    hits, N = clf.loo_curve(8)
    assert N == 30 and hits[0] == 12 and hits[1] == hits[2] == hits[3] == 24 == hits.max()
    best, acc = clf.select_k(8)
    assert best == 2
    assert acc.dtype == np.float64 and acc.shape == (8,)
    np.testing.assert_array_equal(acc, hits / 30)
    # the documented entry point
    best32, acc32 = KNNClassifier(device=device).fit(*dataset("triples")[:2]).select_k(32)
    assert 1 <= best32 <= 32 and acc32.shape == (32,) and acc32[best32 - 1] == acc32.max()


@pytest.mark.parametrize("device", DEVICES)
def test_exact_gives_the_same_bits(device):
    for name in ("triples", "block"):
        clf, kmax = _fit(device, name, exact=True)
        D, I, H = loo_ref(name)
        d, i = clf.loo_kneighbors(kmax)
        np.testing.assert_array_equal(i, I)
        np.testing.assert_array_equal(d, D)
        np.testing.assert_array_equal(clf.loo_curve(kmax, batch_rows=100)[0], H)
    clf, _ = _fit(device, "triples", exact=True)
    fast, _ = _fit(device, "triples")
    Q = np.round(np.random.default_rng(7).uniform(0, 10, (130, 5)), 3)
    np.testing.assert_array_equal(clf.predict_curve(Q, 20), fast.predict_curve(Q, 20))
