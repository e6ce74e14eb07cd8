"""The CPU twin of the weighted vote curve (dmlp_cpu_vote_curve_weighted) against the plain-Python
reference of tests/helpers/weighted_curve_contract.py, bit for bit, and both against what the
library already had: the uniform curve (mode 0) and dmlp_cpu_vote_scores on every prefix of every
sorted row (mode 1) — label and winning score.  A right-to-left sum must change the order-sensitive
rows, so the reference's order is the contract's, not an accident."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.ops import knn as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import result_contract as RC  # noqa: E402
import weighted_curve_contract as WC  # noqa: E402

SPACES = list(RC.LABEL_SPACES)
FILL_I, FILL_D = -12345, -7.0


def cpu_curve(L, kcap, mode, skip=True, truth=True, lists=True, score=True, hits=None, nq=None,
              kstride=None, d_null=False):
    """dmlp_cpu_vote_curve_weighted through ctypes into pre-filled arrays: (rc, label, score, hits,
    (dist, ids))."""
    Q, ks = L["ids"].shape
    ids, dist, k = (np.ascontiguousarray(L[n]) for n in ("ids", "dist", "k"))
    labels, sk, tr = (np.ascontiguousarray(L[n]) for n in ("labels", "skip", "truth"))
    lab = np.full((Q, kcap), FILL_I, np.int32)
    sc = np.full((Q, kcap), FILL_D, np.float64)
    od = np.full((Q, kcap), FILL_D, np.float64)
    oi = np.full((Q, kcap), FILL_I, np.int32)
    hits = np.zeros(kcap, np.uint64) if hits is None else hits
    p = lambda a, on=True: a.ctypes.data if on else None   # noqa: E731
    rc = _lib.lib().dmlp_cpu_vote_curve_weighted(
        p(dist, not d_null), p(ids), ks if kstride is None else kstride, p(k),
        Q if nq is None else nq, p(sk, skip), p(labels), mode, kcap, p(lab), p(sc, score),
        p(od, lists), p(oi, lists), p(tr, truth), p(hits, truth))
    return rc, lab, sc, hits, (od, oi)


def assert_matches(got, ref, ctx, hits_times=1):
    rc, lab, sc, hits, (od, oi) = got
    assert rc == 0, ctx
    np.testing.assert_array_equal(lab, ref[0], err_msg=f"{ctx}: labels")
    np.testing.assert_array_equal(sc.view(np.int64), ref[1].view(np.int64), err_msg=f"{ctx}: scores")
    np.testing.assert_array_equal(hits.astype(np.int64), hits_times * ref[2], err_msg=f"{ctx}: hits")
    np.testing.assert_array_equal(oi, ref[3][1], err_msg=f"{ctx}: ids")
    np.testing.assert_array_equal(od, ref[3][0], err_msg=f"{ctx}: dist")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("space", SPACES)
def test_twin_equals_the_reference(space, mode):
    i = SPACES.index(space)
    kcap, kstride = [(64, 65), (33, 300), (256, 257), (8, 64)][i % 4]
    L, ref = WC.case(kcap, kstride, 42, space, mode, seed=i)
    assert_matches(cpu_curve(L, kcap, mode), ref, f"{space} mode {mode}")
    L0, ref0 = WC.case(kcap, kstride, 42, space, mode, seed=i, with_skip=False)
    assert_matches(cpu_curve(L0, kcap, mode, skip=False), ref0, f"{space} mode {mode}, null skip")
    assert (ref0[0] != ref[0]).any() and 0 < ref[2].sum() < kcap * L["ids"].shape[0]


def test_special_rows():
    """What each special row pins, spelled out on the twin's output."""
    L, ref = WC.case(256, 300, 6, "ten", 1)
    got = cpu_curve(L, 256, 1)
    assert_matches(got, ref, "special rows")
    lab, sc = got[1], got[2]
    a, b = int(L["labels"].max()), int(L["labels"].min())
    row = L["names"]
    for name, at in L["order_at"].items():
        assert lab[row[name], at + 4] == b and lab[row[name], at + 3] == b, name
        assert sc[row[name], at + 4] == 2.0 ** 53 + 2
    assert set(L["order_at"]) == {"order", "order_mid", "order_end"}
    assert L["order_at"]["order_end"] + 5 == 256
    assert list(lab[row["subnormal"], :3]) == [a, a, b] and np.isinf(sc[row["subnormal"], :3]).all()
    assert list(lab[row["inf_label"], :2]) == [b, a]
    assert list(lab[row["huge"], :3]) == [b, b, b] and 0 < sc[row["huge"], 0] < 2.3e-308
    assert list(lab[row["all_inf"], :4]) == [a, a, b, b] and (sc[row["all_inf"]] == 0).all()
    assert list(lab[row["tie"], :2]) == [b, a]
    assert list(lab[row["flip"], :8]) == [b, a] * 4
    assert list(sc[row["unsorted"], :3]) == [1.0, np.inf, np.inf]
    assert (lab[row["nothing"]] == -1).all() and (sc[row["nothing"]] == 0).all()
    assert list(lab[row["skip_zero"], :2]) == [b, b] and list(sc[row["skip_zero"], :2]) == [1.0, 1.0]
    # rows that repeat their last slot
    assert (lab[row["tie"], 2:] == a).all() and (sc[row["tie"], 2:] == 0.5).all()


@pytest.mark.parametrize("space", SPACES)
def test_mode0_is_the_uniform_curve(space):
    L, ref = WC.case(64, 65, 42, space, 0)
    got = cpu_curve(L, 64, 0)
    lab, hits, (od, oi) = K.vote_curve_cpu(L["ids"], L["k"], L["labels"], 64, skip=L["skip"],
                                           truth=L["truth"], dist=L["dist"])
    np.testing.assert_array_equal(got[1], lab)
    np.testing.assert_array_equal(got[3].astype(np.int64), hits)
    np.testing.assert_array_equal(got[4][0], od)
    np.testing.assert_array_equal(got[4][1], oi)
    # the score is the winner's count
    m = (oi >= 0).sum(axis=1)
    for q in range(len(m)):
        for j in range(m[q]):
            assert got[2][q, j] == (L["labels"][oi[q, :j + 1]] == lab[q, j]).sum()


@pytest.mark.parametrize("space", [s for s in SPACES
                                   if 1 <= RC.label_space(s, 4)[2] - RC.label_space(s, 4)[1] <= 4096])
def test_mode1_is_vote_scores_at_every_prefix(space):
    """On a sorted row with every label in range, column j is dmlp_cpu_vote_scores' winner — label
    and score bits — on the first j + 1 kept entries."""
    kcap, kstride = 33, 300
    L, _ = WC.case(kcap, kstride, 42, space, 1)
    _, lo, hi = RC.label_space(space, WC.N_IDS, 0)
    _, lab, sc, _, (od, oi) = cpu_curve(L, kcap, 1)
    rows = np.flatnonzero(WC.sorted_rows(L, kcap))
    assert len(rows) >= 42 and not WC.sorted_rows(L, kcap)[L["names"]["unsorted"]]
    for j in range(kcap):
        kk = np.full(len(rows), j + 1, np.int32)
        _, s, l = K.vote_scores_cpu(oi[rows], kk, L["labels"], lo, hi - lo, "inv_sqdist",
                                    dist=od[rows])
        np.testing.assert_array_equal(l, lab[rows, j], err_msg=f"prefix {j + 1}")
        full = oi[rows, 0] >= 0          # (-1 is a label of some spaces)
        win = s[np.flatnonzero(full), l[full] - lo]
        np.testing.assert_array_equal(win.view(np.int64), sc[rows[full], j].view(np.int64),
                                      err_msg=f"prefix {j + 1}")
        assert (sc[rows[~full], j] == 0).all()


def test_right_to_left_changes_the_order_rows():
    L, ref = WC.case(256, 300, 6, "ten", 1)
    wrong = WC.curve_ref(L["ids"], L["k"], L["labels"], 256, 1, L["dist"], L["skip"], r2l=True)
    twin = cpu_curve(L, 256, 1)[1]
    a = int(L["labels"].max())
    assert len(L["order_at"]) == 3
    for name, at in L["order_at"].items():
        r, col = L["names"][name], at + WC.ORDER_COLUMN
        assert wrong[0][r, col] == a != ref[0][r, col] == twin[r, col], name
        assert (wrong[0][r, :col] == ref[0][r, :col]).all(), name


def test_argument_errors_write_nothing():
    L, _ = WC.case(8, 64, 5, "ten", 1)
    hits = np.full(8, 3, np.uint64)

    def untouched(got, rc):
        assert got[0] == rc
        assert (got[1] == FILL_I).all() and (got[2] == FILL_D).all() and (hits == 3).all()
        assert (got[4][0] == FILL_D).all() and (got[4][1] == FILL_I).all()
    for mode in (-1, 2):
        untouched(cpu_curve(L, 8, mode, hits=hits), -1)
    untouched(cpu_curve(L, 8, 1, hits=hits, d_null=True, lists=False), -1)
    untouched(cpu_curve(L, 8, 0, hits=hits, d_null=True), -1)       # lists without d
    untouched(cpu_curve(L, 8, 1, hits=hits, kstride=0), -1)
    untouched(cpu_curve(L, 8, 1, hits=hits, nq=0), 0)
    untouched(cpu_curve(L, 8, 1, hits=hits, nq=-2), 0)
    Lb = _lib.lib()
    ids, k, lab = np.zeros((1, 4), np.int32), np.ones(1, np.int32), np.zeros(4, np.int32)
    out = np.full(300, FILL_I, np.int32)
    d = np.ones((1, 4))
    for kcap in (0, 257, -1):
        assert Lb.dmlp_cpu_vote_curve_weighted(d.ctypes.data, ids.ctypes.data, 4, k.ctypes.data, 1,
                                               None, lab.ctypes.data, 1, kcap, out.ctypes.data,
                                               None, None, None, None, None) == -1
    # half-given pairs
    assert Lb.dmlp_cpu_vote_curve_weighted(d.ctypes.data, ids.ctypes.data, 4, k.ctypes.data, 1, None,
                                           lab.ctypes.data, 1, 4, out.ctypes.data, None,
                                           d.ctypes.data, None, None, None) == -1
    assert Lb.dmlp_cpu_vote_curve_weighted(d.ctypes.data, ids.ctypes.data, 4, k.ctypes.data, 1, None,
                                           lab.ctypes.data, 1, 4, out.ctypes.data, None, None,
                                           None, k.ctypes.data, None) == -1
    assert (out == FILL_I).all()
    # a null d is fine in mode 0 without the lists
    got = cpu_curve(L, 8, 0, d_null=True, lists=False)
    assert got[0] == 0 and (got[1] != FILL_I).all() and (got[4][1] == FILL_I).all()


def test_ops_wrapper():
    """vote_curve_cpu: the defaults take the old entry, weights / score the new one."""
    L, ref = WC.case(8, 64, 5, "ten", 1)
    args = (L["ids"], L["k"], L["labels"], 8)
    kw = dict(skip=L["skip"], truth=L["truth"], dist=L["dist"])
    lab, hits, (od, oi), sc = K.vote_curve_cpu(*args, **kw, weights="inv_sqdist", score=True)
    np.testing.assert_array_equal(lab, ref[0])
    np.testing.assert_array_equal(sc.view(np.int64), ref[1].view(np.int64))
    np.testing.assert_array_equal(hits, ref[2])
    np.testing.assert_array_equal(oi, ref[3][1])
    out = K.vote_curve_cpu(*args, **kw, weights="inv_sqdist")
    assert len(out) == 3 and (out[0] == lab).all()
    assert K.vote_curve_cpu(*args, **kw, weights="inv_sqdist", lists=False)[2] is None
    base = K.vote_curve_cpu(*args, **kw)
    uni = K.vote_curve_cpu(*args, **kw, score=True)
    assert len(base) == 3 and len(uni) == 4 and (base[0] == uni[0]).all()
    assert (uni[3] >= 0).all() and (uni[3] == np.floor(uni[3])).all()
    with pytest.raises(ValueError):
        K.vote_curve_cpu(*args, skip=L["skip"], weights="inv_sqdist")      # no dist
    with pytest.raises(ValueError):
        K.vote_curve_cpu(*args, **kw, weights="distance")
