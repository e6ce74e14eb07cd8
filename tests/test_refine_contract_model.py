"""Pins tests/helpers/refine_contract.py — the hand-built candidate lists and the float64 reference
the GPU test of the refine kernels compares with — before it judges a kernel.  No GPU.

  * the reference's list of every case equals dmlp_cpu_knn over the survivor rows alone, its label
    and checksum dmlp_cpu_finalize;
  * a_model equals the score recomputed from the words of the host-rendered image;
  * group_rows / group_of_row round-trip;
  * every case moves (status or a list slot of some query) under each mutant of the rule it is
    aimed at, and every mutant is aimed at by some case of every family it applies to."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd.ops import knn as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import refine_contract as RF  # noqa: E402
import result_contract as RC  # noqa: E402
import x1_contract as X1  # noqa: E402

FAMILIES = "ABCDEFG"


def family(f):
    return [c for c in RF.cases().values() if c.family == f]


@pytest.mark.parametrize("f", FAMILIES)
def test_reference_is_cpu_knn_of_the_survivors(f):
    """Rows in ascending id, so that dmlp_cpu_knn's id-descending tie rule carries over; ids
    mapped back.  A handed-back query has no list."""
    for case in family(f):
        res = RF.refine_ref(case)
        pr = case.prob
        for p, q in enumerate(case.rows):
            kq = int(case.k[q])
            if res.status[p]:
                assert res.surv[p] is None or len(res.surv[p]) > case.v.capacity
                continue
            rows = np.sort(res.surv[p])
            assert len(np.unique(rows)) == len(rows) == res.nsurv[p], case.name
            n = min(kq, len(rows))
            assert (res.i[p, n:] == -1).all() and np.isposinf(res.d[p, n:]).all()
            if n == 0:
                continue
            d, i = K.knn_cpu(pr.X[rows], pr.Qx[q:q + 1], np.array([kq], np.int32),
                             kstride=case.kstride, nthreads=1)
            np.testing.assert_array_equal(res.i[p, :n], rows[i[0, :n]], err_msg=case.name)
            np.testing.assert_array_equal(res.d[p, :n], d[0, :n], err_msg=case.name)


@pytest.mark.parametrize("f", FAMILIES)
def test_reference_vote_and_checksum(f):
    for case in family(f):
        if not case.labels:
            continue
        res = RF.refine_ref(case)
        lab, cs = K.finalize_cpu(res.i, case.k[case.rows], case.label_space()[0])
        np.testing.assert_array_equal(res.label, lab, err_msg=case.name)
        np.testing.assert_array_equal(res.cs, cs, err_msg=case.name)


def test_a_model_is_the_image():
    """The float64 score of the words the kernels read (tile image, xinit, query fragments) is
    a_model: the margin the builder keeps is taken against the right numbers."""
    seen = {}
    for case in RF.cases().values():
        if case.prob.hl == 1:
            seen[case.prob.key] = case.prob
    assert len(seen) >= 10
    for pr in seen.values():
        img = RF.image_scores(pr.ref)
        scale = np.abs(pr.score).max()
        assert np.abs(img - pr.score).max() <= 1e-12 * scale, pr.key   # float64 summation order
        assert float(pr.eps.min()) > 1e6 * 1e-12 * scale


@pytest.mark.parametrize("grows", [4, 8])
def test_group_geometry_round_trips(grows):
    n_tiles = 5
    gi = np.arange(X1.n_groups(n_tiles, grows))
    rows = X1.group_rows(gi, grows)
    assert sorted(rows.reshape(-1).tolist()) == list(range(n_tiles * 64))   # a partition
    assert (X1.group_of_row(rows, grows) == gi[:, None]).all()
    assert (X1.group_of_row(np.arange(n_tiles * 64), grows) < len(gi)).all()
    if grows == 8:   # rows 4 kg + i of two 16-row steps
        assert rows[5].tolist() == [36, 37, 38, 39, 52, 53, 54, 55]
    else:
        assert rows[5].tolist() == [20, 21, 22, 23]


def test_margin_holds_for_every_case():
    """No listed member's score lies within MARGIN eps of the threshold in force (Builder.done
    asserts it while building; here it is recomputed from the finished lists)."""
    for case in RF.cases().values():
        v = case.v
        if not v.image:
            continue
        pr = case.prob
        for p, q in enumerate(case.rows):
            if (case.cnt[p] < 0).any() or case.hq[p] == -np.inf:
                continue
            for s in range(case.S):
                e = case.ids[p, s, :case.cnt[p, s]].view(np.uint32).astype(np.int64)
                rows = (s * case.tps * 64 + X1.group_rows(e & 0xFFFF, case.grows)).reshape(-1)
                rows = rows[rows < pr.N]
                assert (np.abs(pr.score[q, rows] - np.float64(case.hq[p])) > pr.eps[q]).all(), \
                    f"{case.name}: query {q} slice {s}"


# mutant -> the families that must hold a case aimed at it
AIMED_IN = {
    "cap_minus": "AC", "cap_plus": "AC", "no_threshold": "CD", "no_2eps": "D", "eps_slice0": "D",
    "kth_distinct": "D", "no_cut": "E", "to_cap": "ABCDEFG", "swap_grows": "A", "r2l": "B",
    "id_asc": "BG",
}


@pytest.mark.parametrize("f", FAMILIES)
def test_cases_discriminate(f):
    """Each case changes status or a list slot of some query under every mutant it is aimed at."""
    for case in family(f):
        base = RF.refine_ref(case)
        for m in case.aimed:
            assert base.differs(RF.refine_ref(case, RF.MUTANTS[m]), case.k), \
                f"{case.name} does not move under {m}"


@pytest.mark.parametrize("mutant", list(RF.MUTANTS))
def test_every_mutant_is_aimed_at(mutant):
    for f in AIMED_IN[mutant]:
        assert any(mutant in c.aimed for c in family(f)), f"no case of family {f} aims at {mutant}"


def test_families_reach_their_branches():
    """The shapes the families promise, counted from the reference."""
    c = RF.cases()
    for name, C in (("pair", 64), ("groups", 128), ("groups2", 128), ("collect", 512), ("exact", 512)):
        A = 40 if name == "groups2" else 32
        one, most = RF.refine_ref(c[f"A-{name}-A{A}-N{RF.N_ONE}"]), RF.refine_ref(c[f"A-{name}-A{A}-N{RF.N_MOST}"])
        assert one.nsurv.tolist() == [C, C + 1, C, C + 1, C] and one.status.tolist() == [0, 1, 0, 1, 0]
        assert most.nsurv.tolist() == [C - 1, C, C - 1, C, C - 1] and not most.status.any()
        thr = RF.refine_ref(c[f"C-{name}-A{A}"]) if name != "exact" else None
        if thr is not None:
            assert thr.nsurv.tolist() == [5, C, C + 1, 3, 10] and thr.status.tolist() == [0, 0, 1, 0, 0]
    for name in ("groups", "groups2"):
        res = RF.refine_ref(c[f"D-eps-{name}"])
        assert (res.status == 1).all() and (res.nsurv > 128).all()
        pre = c[f"B-prefilter-{name}"]
        res = RF.refine_ref(pre)
        for p, q in enumerate(pre.rows):   # every neighbour past candidate position 64
            pos = {r: j for j, r in enumerate(res.surv[p].tolist())}
            assert 64 < len(pos) <= 128 and min(pos[r] for r in res.i[p, :pre.k[q]]) >= 64
    for cap, P in ((128, 256), (256, 256), (512, 512)):
        g = c[f"G-refine-cap{cap}-S4-A9"]
        M = g.cnt.clip(0).sum(axis=1)
        assert M[3] > P and M[0] <= 64 < M[1] <= P and g.k[1] <= 64 < g.k[2] <= 128
    assert c["G-refine-cap512-S4-A9"].k[3] == 256
    inf = RF.refine_ref(c["B-inf-exact"])
    assert np.isposinf(inf.d[0, 13:16]).all() and (inf.i[0, 13:16] >= 0).all() and inf.i[0, 16] == -1
