"""Pins tests/helpers/vote_curve_contract.py (the NumPy / Python-integer reference of the vote
curve) against the CPU twin dmlp_cpu_vote_curve, and both against dmlp_cpu_finalize — the twin
that existed before the curve — at every prefix.  No GPU."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.ops import knn as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import result_contract as RC  # noqa: E402
import vote_curve_contract as VC  # noqa: E402

KCAP, KSTRIDE, NQ = 33, 34, 42   # 42 rows: every (recipe, k choice) pair


def _twin(L, kcap, skip=True, truth=True, lists=True, hits=None):
    return K.vote_curve_cpu(L["ids"], L["k"], L["labels"], kcap, skip=L["skip"] if skip else None,
                            truth=L["truth"] if truth else None,
                            dist=L["dist"] if lists else None, hits=hits)


def _assert_same(got, ref, ctx):
    np.testing.assert_array_equal(got[0], ref[0], err_msg=f"{ctx}: labels")
    np.testing.assert_array_equal(got[1], ref[1], err_msg=f"{ctx}: hits")
    np.testing.assert_array_equal(got[2][1], ref[2][1], err_msg=f"{ctx}: ids")
    np.testing.assert_array_equal(got[2][0], ref[2][0], err_msg=f"{ctx}: dist")


@pytest.mark.parametrize("space", list(RC.LABEL_SPACES))
def test_curve_ref_matches_cpu_twin_and_finalize(space):
    L, ref = VC.case(KCAP, KSTRIDE, NQ, space)
    got = _twin(L, KCAP)
    _assert_same(got, ref, space)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64
    # the pre-existing twin on the self-excluded list: its vote at k is column k - 1
    oi = ref[2][1]
    for kk in range(1, KCAP + 1):
        lab, _ = K.finalize_cpu(oi, np.full(NQ, kk, np.int32), L["labels"])
        np.testing.assert_array_equal(lab, ref[0][:, kk - 1], err_msg=f"{space} k={kk}")


@pytest.mark.parametrize("space", ["ten", "extreme", "distinct"])
def test_curve_without_skip_is_finalize_of_the_raw_list(space):
    """Null skip: column k - 1 is dmlp_cpu_finalize of the list itself at min(k, k_q, 256), on
    every row whose padding sits in the tail."""
    L, ref = VC.case(KCAP, KSTRIDE, NQ, space, with_skip=False)
    got = _twin(L, KCAP, skip=False)
    _assert_same(got, ref, space)
    rows = ~L["mid_negative"]
    for kk in range(1, KCAP + 1):
        kq = np.minimum(kk, np.clip(L["k"], 0, None)).astype(np.int32)
        lab, _ = K.finalize_cpu(L["ids"], kq, L["labels"])
        np.testing.assert_array_equal(lab[rows], got[0][rows, kk - 1], err_msg=f"k={kk}")


@pytest.mark.parametrize("kcap,kstride", [(1, 1), (2, 3), (31, 300), (64, 64), (65, 66),
                                           (255, 256), (256, 256), (256, 300)])
def test_curve_ref_matches_cpu_twin_shapes(kcap, kstride):
    """The shapes of the GPU contract test, the 256-slot clamp of a 300-wide list included."""
    L, ref = VC.case(kcap, kstride, 7, "r257", seed=kcap % 7)
    _assert_same(_twin(L, kcap), ref, f"kcap {kcap} kstride {kstride}")


def test_clamp_to_256_slots():
    """A 300-wide list with k = 300: only the first 256 slots vote."""
    rng = np.random.default_rng(0)
    labels = rng.integers(0, 3, 600).astype(np.int32)
    ids = rng.permutation(600)[:300].astype(np.int32)[None, :]
    lab, _, _ = K.vote_curve_cpu(ids, [300], labels, 256)
    assert lab[0, 255] == RC.vote_ref(ids[0], 256, labels)
    # the skipped id makes room for no slot past 255
    lab2, _, (_, oi) = K.vote_curve_cpu(ids, [300], labels, 256, skip=ids[0, :1],
                                        dist=np.zeros((1, 300)))
    assert oi[0, 254] == ids[0, 255] and oi[0, 255] == -1 and lab2[0, 255] == lab2[0, 254]


def test_hits_accumulate_and_null_pairs():
    L, ref = VC.case(KCAP, KSTRIDE, NQ, "ten")
    lab, hits, lists = _twin(L, KCAP, truth=False, lists=False)
    assert hits is None and lists is None
    np.testing.assert_array_equal(lab, ref[0])
    _, h1, _ = _twin(L, KCAP, lists=False)
    _, h2, _ = _twin(L, KCAP, lists=False, hits=h1.copy())
    np.testing.assert_array_equal(h1, ref[1])
    np.testing.assert_array_equal(h2, 2 * ref[1])
    assert 0 < ref[1].sum() < NQ * KCAP


def test_argument_errors():
    Lb = _lib.lib()
    ids = np.zeros((2, 4), np.int32)
    k = np.full(2, 4, np.int32)
    labels = np.zeros(1, np.int32)
    out = np.full((2, 4), -12345, np.int32)
    od = np.full((2, 4), -7.0)
    hits = np.full(4, -12345, np.int64)

    def call(kstride=4, nq=2, kcap=4, d=od, o_d=None, o_i=None, truth=None, h=None):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return Lb.dmlp_cpu_vote_curve(p(d), p(ids), kstride, p(k), nq, None, p(labels), kcap,
                                      p(out), p(o_d), p(o_i), p(truth), p(h))
    assert call(kcap=0) == -1 and call(kcap=257) == -1 and call(kstride=0) == -1
    assert call(o_d=od) == -1 and call(o_i=out) == -1
    assert call(truth=k) == -1 and call(h=hits) == -1
    assert call(nq=0) == 0
    assert (out == -12345).all() and (hits == -12345).all() and (od == -7.0).all()
    assert call() == 0 and (out == 0).all()
    with pytest.raises(ValueError):
        K.vote_curve_cpu(ids, k, labels, 257)
