"""predict_proba and the weighted predict of KNNClassifier — the CPU path here, the same cases on
the GPU path (the class-score kernel behind the native search) under `gpu`.  The oracle is a brute
force that shares nothing with the engine but the host normalisation: result_contract.knn_ref's
lists (left-to-right distances, (dist asc, id desc) order), vote_scores_contract.scores_ref on them,
then ops.knn.class_proba.  All comparisons are bit-exact."""
import functools
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd.models import KNNClassifier
from distributed_machine_learning_project_amd.ops import knn as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import result_contract as RC  # noqa: E402
import vote_scores_contract as VS  # noqa: E402

DEVICES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]
WEIGHTS = ("uniform", "inv_sqdist")
N, A, NQ = 600, 8, 40
LO, NCLASS = -3, 7


@functools.lru_cache(maxsize=None)
def dataset():
    """(X [600, 8], y, Q [40, 8]): attributes in {0, 1, 2}, so distances are small integers with
    many ties, rows repeat (ten copies of row 100 among them, labelled independently) and zero
    distances occur; 7 labels from -3; the first 12 queries are training rows, 100 included."""
    rng = np.random.default_rng(11)
    X = rng.integers(0, 3, (N, A)).astype(np.float64)
    X[100:110] = X[100]
    y = rng.integers(LO, LO + NCLASS, N).astype(np.int32)
    y[:2] = LO, LO + NCLASS - 1
    Q = rng.integers(0, 3, (NQ, A)).astype(np.float64)
    Q[:12] = X[[100, 0, 7, 599, 250, 31, 32, 33, 400, 401, 105, 2]]
    for a in (X, y, Q):
        a.setflags(write=False)
    return X, y, Q


def k_array():
    return np.array([1, 5, 64, 300, 2, 600, 700, 0, 17, 256] * 4, np.int32)[:NQ]


@functools.lru_cache(maxsize=None)
def brute(k, weights):
    """(proba, label, count) of the brute force; k an int, or "array" for k_array()."""
    X, y, Q = dataset()
    kk = k_array() if k == "array" else np.full(NQ, k, np.int32)
    d, i = RC.knn_ref(X, Q, kk, max(1, int(kk.max())))
    cnt, sc, lab = VS.scores_ref(i, kk, y, LO, NCLASS, WEIGHTS.index(weights), d)
    p = K.class_proba(sc, cnt)
    for a in (p, lab, cnt):
        a.setflags(write=False)
    return p, lab, cnt


@functools.lru_cache(maxsize=None)
def fitted(device):
    X, y, _ = dataset()
    return KNNClassifier(device=device).fit(X, y)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("k", [1, 5, 64, 300, "array"])
def test_predict_proba_matches_brute_force(device, weights, k):
    clf = fitted(device)
    Q = dataset()[2]
    np.testing.assert_array_equal(clf.classes_, np.arange(LO, LO + NCLASS))
    p = clf.predict_proba(Q, k_array() if k == "array" else k, weights=weights)
    ref, lab, cnt = brute(k, weights)
    assert p.dtype == np.float64 and p.shape == (NQ, NCLASS)
    np.testing.assert_array_equal(p.view(np.int64), ref.view(np.int64))
    m = cnt.sum(axis=1)
    full = m > 0
    if weights == "uniform":    # an integer check: the shares are count / m
        np.testing.assert_array_equal(p[full], cnt[full] / m[full, None])
        np.testing.assert_array_equal(m, np.minimum(np.full(NQ, k) if k != "array" else k_array(),
                                                    N))
    np.testing.assert_allclose(p[full].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert (p[~full] == 0).all() and (full.all() or k == "array")
    np.testing.assert_array_equal(clf.predict(Q, k_array() if k == "array" else k, weights=weights),
                                  lab)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("k", [1, 5, 64])
def test_coinciding_queries_see_only_their_twins(device, k):
    """A query equal to training rows: with inverse-distance weights the probability lies on the
    classes of the rows at distance 0 among its k neighbours, in the shares of their counts."""
    X, y, Q = dataset()
    clf = fitted(device)
    p = clf.predict_proba(Q[:12], k, weights="inv_sqdist")
    for q in range(12):
        twins = np.flatnonzero((X == Q[q]).all(axis=1))[::-1][:k]    # (id desc among equals)
        want = np.bincount(y[twins] - LO, minlength=NCLASS) / len(twins)
        np.testing.assert_array_equal(p[q], want, err_msg=f"query {q}")
    assert len(np.flatnonzero((X == Q[0]).all(axis=1))) >= 10


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("k", [1, 5, 64, 300, "array"])
def test_predict_is_unchanged(device, k):
    """predict(Q, k) is predict(Q, k, weights="uniform") and the argmax of the uniform shares
    under the tie rule (the larger label)."""
    clf = fitted(device)
    Q = dataset()[2]
    kk = k_array() if k == "array" else k
    lab = clf.predict(Q, kk)
    np.testing.assert_array_equal(lab, clf.predict(Q, kk, weights="uniform"))
    p, ref, cnt = brute(k, "uniform")
    np.testing.assert_array_equal(lab, ref)
    last = NCLASS - 1 - np.argmax(p[:, ::-1], axis=1)     # the last of the largest shares
    want = np.where(cnt.sum(axis=1) > 0, clf.classes_[last], -1)
    np.testing.assert_array_equal(lab, want)


@pytest.mark.gpu
@pytest.mark.parametrize("weights", WEIGHTS)
def test_cpu_and_gpu_agree_bit_for_bit(weights):
    Q = dataset()[2]
    cpu, gpu = fitted("cpu"), fitted("gpu")
    for k in (1, 5, 64, 300, k_array()):
        a, b = cpu.predict_proba(Q, k, weights=weights), gpu.predict_proba(Q, k, weights=weights)
        np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))
        np.testing.assert_array_equal(cpu.predict(Q, k, weights=weights),
                                      gpu.predict(Q, k, weights=weights))


@pytest.mark.parametrize("device", DEVICES)
def test_value_errors(device):
    clf = fitted(device)
    X, y, Q = dataset()
    with pytest.raises(ValueError):
        clf.predict_proba(Q, 5, weights="distance")
    with pytest.raises(ValueError):
        clf.predict(Q, 5, weights="distance")
    # a label range past the class-score limit: what existed before still works
    wide = y.copy()
    wide[1] = LO + K.VOTE_SCORES_CMAX      # (wide[0] is LO: one value more than the limit)
    big = KNNClassifier(device=device).fit(X, wide)
    np.testing.assert_array_equal(big.predict(Q, 5), RC.finalize_ref(
        RC.knn_ref(X, Q, np.full(NQ, 5), 5)[1], np.full(NQ, 5), wide)[0])
    assert big.predict_curve(Q, 3).shape == (NQ, 3)
    for call in (lambda: big.classes_, lambda: big.predict_proba(Q, 5),
                 lambda: big.predict(Q, 5, weights="inv_sqdist")):
        with pytest.raises(ValueError):
            call()
    # exactly the limit fits
    wide[1] = LO + K.VOTE_SCORES_CMAX - 1
    fits = KNNClassifier(device=device).fit(X, wide)
    assert fits.predict_proba(Q[:3], 5).shape == (3, K.VOTE_SCORES_CMAX)
