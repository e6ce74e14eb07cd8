"""What KNNClassifier and KNNRegressor share (models/_knn_base.py) and the argument checks the eight
list-kernel wrappers of ops.knn share: row selection of the leave-one-out calls (negative ids,
stepped slices, repeated ids, empty selections), the two estimators' searches agreeing with each
other after the same update, empty query batches, and for every wrapper the arguments it must
refuse and one call that must not depend on its inputs being contiguous.  Comparisons are on bits
(NaN == NaN); the GPU cases are the same cases behind `gpu`."""
import functools

import numpy as np
import pytest

from distributed_machine_learning_project_amd import Update
from distributed_machine_learning_project_amd.models import KNNClassifier, KNNRegressor
from distributed_machine_learning_project_amd.ops import knn as K

DEVICES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]
N, A, NQ, KMAX = 40, 4, 6, 5


@functools.lru_cache(maxsize=None)
def dataset():
    """(X [40, 4], labels [40] in 3 classes, targets [40], Q [6, 4]), rounded to 3 decimals."""
    rng = np.random.default_rng(23)
    X = np.round(rng.uniform(0.0, 10.0, (N, A)), 3)
    y = rng.integers(0, 3, N).astype(np.int32)
    t = np.round(rng.uniform(-5.0, 5.0, N), 3)
    Q = np.round(rng.uniform(0.0, 10.0, (NQ, A)), 3)
    for a in (X, y, t, Q):
        a.setflags(write=False)
    return X, y, t, Q


@functools.lru_cache(maxsize=None)
def fitted(device):
    X, y, t, _ = dataset()
    return KNNClassifier(device=device).fit(X, y), KNNRegressor(device=device).fit(X, t)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def loo_calls(device):
    """rows -> tuple of arrays with one row per selected dataset row, for both estimators."""
    clf, reg = fitted(device)
    return (lambda rows: clf.loo_kneighbors(KMAX, rows=rows),
            lambda rows: (reg.loo_predict_curve(KMAX, rows=rows),),
            lambda rows: (reg.loo_predict_curve(KMAX, rows=rows, weights="inv_sqdist"),))


# ------------------------------------------------------------------ leave-one-out row selection
@pytest.mark.parametrize("device", DEVICES)
def test_negative_row_ids(device):
    for call in loo_calls(device):
        for got, want in zip(call([-1, -N, 3]), call([N - 1, 0, 3])):
            assert want.shape[:2] == (3, KMAX) and same(got, want)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("rows", [slice(1, 30, 2), slice(None, None, 13), np.array([7, 7, 2, 39, 7])],
                         ids=["step2", "step13", "repeated"])
def test_stepped_and_repeated_rows(device, rows):
    ids = np.arange(N)[rows]
    for call in loo_calls(device):
        got = call(rows)
        for j, r in enumerate(ids):
            for g, one in zip(got, call([int(r)])):
                assert g.shape[:2] == (len(ids), KMAX) and same(g[j:j + 1], one)


@pytest.mark.parametrize("rows", [[], np.zeros(0, np.int64), slice(3, 3)],
                         ids=["list", "array", "slice"])
def test_empty_row_selection(rows):
    clf, reg = fitted("cpu")
    d, i = clf.loo_kneighbors(KMAX, rows=rows)
    assert d.shape == i.shape == (0, KMAX) and d.dtype == np.float64 and i.dtype == np.int32
    assert reg.loo_predict_curve(KMAX, rows=rows).shape == (0, KMAX)


def test_empty_query_batch():
    clf, reg = fitted("cpu")
    Q = np.zeros((0, A))
    assert clf.predict(Q, 3).shape == (0,)
    assert clf.predict_curve(Q, KMAX).shape == (0, KMAX)
    assert clf.predict_proba(Q, 3).shape == (0, len(clf.classes_))
    assert reg.predict(Q, 3).shape == (0,)
    assert reg.predict_curve(Q, KMAX).shape == (0, KMAX)


# ------------------------------------------------------------------ the two estimators, one search
@pytest.mark.parametrize("device", DEVICES)
def test_estimators_search_alike_after_update(device):
    X, y, t, Q = dataset()
    clf = KNNClassifier(device=device).fit(X.copy(), y)
    reg = KNNRegressor(device=device).fit(X.copy(), t)
    ups = [Update(3, list(Q[0] + 0.001)), Update(17, list(Q[1])), Update(3, list(Q[2] - 0.001))]
    for k in (4, np.array([1, 40, 7, 0, 3, 12], np.int32)):
        before = clf.kneighbors(Q, k)
        assert all(same(a, b) for a, b in zip(before, reg.kneighbors(Q, k)))
    assert clf.update(ups) is clf and reg.update(ups) is reg
    for k in (4, np.array([1, 40, 7, 0, 3, 12], np.int32)):
        after = clf.kneighbors(Q, k)
        assert all(same(a, b) for a, b in zip(after, reg.kneighbors(Q, k)))
    assert after[1][1, 0] == 17 and after[0][1, 0] == 0.0   # the update reached the search
    assert same(clf.X, reg.X) and same(clf.X[17], Q[1])


@pytest.mark.parametrize("device", DEVICES)
def test_regressor_on_row_numbers_names_the_classifiers_neighbour(device):
    """At k = 1 the mean of one fp64 integer is that integer: a regressor fitted on y = arange(N)
    returns the id of each row's nearest other row, which the classifier lists in column 0."""
    X = dataset()[0]
    reg = KNNRegressor(device=device).fit(X, np.arange(N, dtype=np.float64))
    ids = fitted(device)[0].loo_kneighbors(1)[1]
    assert ids.shape == (N, 1) and (ids >= 0).all()
    assert same(reg.loo_predict_curve(1), ids.astype(np.float64))


# ------------------------------------------------------------------ the wrappers' argument checks
WRAPPERS = ("vote_curve", "vote_scores", "neighbor_means", "neighbor_means_curve")
HAS_WEIGHTS = WRAPPERS[1:]
HAS_KCAP = ("vote_curve", "neighbor_means_curve")
Q3, KS = 3, 2


def lists():
    """Good arguments at Q = 3, kstride = 2 over 6 dataset rows."""
    return {"ids": np.array([[4, 1], [0, -1], [5, 2]], np.int32),
            "k": np.array([2, 1, 2], np.int32),
            "skip": np.array([-1, 0, 2], np.int32),
            "dist": np.array([[0.5, 1.25], [0.0, np.inf], [2.0, 2.0]], np.float64)}


LABELS = np.array([0, 2, 1, 1, 0, 2], np.int32)
TARGETS = np.array([[1.5], [-2.0], [0.25], [8.0], [3.0], [-0.125]], np.float64)
TRUTH = np.array([0, 0, 2], np.int32)


def put(backend, a):
    if backend == "cpu" or a is None:
        return a
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def call(name, backend, ids, k, *, kcap=2, weights="uniform", **kw):
    f = getattr(K, f"{name}_{backend}")
    if name == "vote_curve":
        return f(ids, k, put(backend, LABELS), kcap, **kw)
    if name == "vote_scores":
        return f(ids, k, put(backend, LABELS), 0, 3, weights, **kw)
    if name == "neighbor_means":
        return f(ids, k, put(backend, TARGETS), weights, **kw)
    return f(ids, k, put(backend, TARGETS), kcap, weights, **kw)


def host(out):
    """The arrays of a wrapper's result, on the host, in order (None kept)."""
    if out is None or isinstance(out, np.ndarray):
        return [out]
    if isinstance(out, tuple):
        return [a for o in out for a in host(o)]
    return [out.cpu().numpy()]


@pytest.mark.parametrize("backend", DEVICES)
@pytest.mark.parametrize("name", WRAPPERS)
def test_wrapper_refuses(name, backend):
    good = {key: put(backend, a) for key, a in lists().items()}
    bad = {
        "ids 1-d": dict(good, ids=good["ids"][0]),
        "k short": dict(good, k=good["k"][:-1]),
        "skip short": dict(good, skip=good["skip"][:-1]),
        "dist narrower": dict(good, dist=good["dist"][:, :1]),
        "dist shorter": dict(good, dist=good["dist"][:-1]),
    }
    if backend == "gpu":
        bad["ids int64"] = dict(good, ids=good["ids"].long())
        bad["dist float32"] = dict(good, dist=good["dist"].float())
    if name in HAS_WEIGHTS:
        bad["weights unknown"] = dict(good, weights="distance")
        bad["inv_sqdist without dist"] = dict(good, weights="inv_sqdist", dist=None)
    if name in HAS_KCAP:
        bad["kcap 0"] = dict(good, kcap=0)
        bad["kcap 257"] = dict(good, kcap=257)
    if name == "vote_curve":
        truth = put(backend, TRUTH)
        bad["truth short"] = dict(good, truth=truth[:-1])
        # what numel() / len() used to let through, and what used to reach the C entry
        bad["k [Q, 1]"] = dict(good, k=good["k"][:, None])
        bad["skip [Q, 1]"] = dict(good, skip=good["skip"][:, None])
        bad["truth [Q, 1]"] = dict(good, truth=truth[:, None])
        bad["kstride 0"] = dict(good, ids=good["ids"][:, :0], dist=None)
    for what, kw in bad.items():
        with pytest.raises(ValueError):
            call(name, backend, **kw)
            pytest.fail(f"{name}_{backend} accepted: {what}")
    call(name, backend, **good)    # and the arguments they were derived from pass


@pytest.mark.parametrize("backend", DEVICES)
@pytest.mark.parametrize("name", WRAPPERS)
def test_wrapper_takes_strided_inputs(name, backend):
    """Columns of a wider array, every other element of a longer one: same bits as packed inputs."""
    L = lists()
    if name in HAS_WEIGHTS:
        L["weights"] = "inv_sqdist"
    if name == "vote_curve":
        L["truth"] = TRUTH
    good = {key: a if isinstance(a, str) else put(backend, a) for key, a in L.items()}
    wide = {key: put(backend, np.concatenate([L[key], 7 - L[key]], axis=1))[:, :KS]
            for key in ("ids", "dist")}
    thin = {key: put(backend, np.repeat(L[key], 2))[::2] for key in ("k", "skip")}
    if backend == "cpu":
        assert not any(a.flags.c_contiguous for a in (*wide.values(), *thin.values()))
    else:
        assert not any(a.is_contiguous() for a in (*wide.values(), *thin.values()))
    want = host(call(name, backend, **good))
    got = host(call(name, backend, **dict(good, **wide, **thin)))
    assert len(got) == len(want) and any(a is not None and a.size for a in want)
    for g, w in zip(got, want):
        assert (g is None and w is None) or same(g, w)
