"""Kernel-level contract of the vote curve (csrc/vote_curve.hip, dmlp.h: dmlp_vote_curve) through
the C ABI.

Every output goes into a buffer of exactly nq * kcap slots between sentinel bands
(tests/helpers/result_contract.py: guarded) and every slot is compared, bit for bit, with the
NumPy / Python-integer reference of tests/helpers/vote_curve_contract.py (pinned against the CPU
twin and dmlp_cpu_finalize by tests/test_vote_curve_model.py).  dmlp_finalize — the kernel a
caller had to launch once per k before — is the second oracle: its vote at k is column k - 1.

The lists (vote_curve_contract.make_lists) rotate seven row recipes (random, alternating a, b, a,
b — the winner changes at every prefix and every even prefix is a count tie —, staircase a, b, c,
all equal, padding in the tail, real entries at +inf, a negative id in the middle), six k choices
(0, 1, kcap - 1, kcap, kcap + 1, > kstride) and five skips (first, middle, last, absent, -1)."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import result_contract as RC  # noqa: E402
import vote_curve_contract as VC  # noqa: E402

pytestmark = pytest.mark.gpu

KCAPS = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256)
SPACES = list(RC.LABEL_SPACES)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()   # (a copy: writable)


class Run:
    """One dmlp_vote_curve call into guarded outputs."""

    def __init__(self, torch, L, kcap, skip=True, truth=True, lists=True, hits=None, nq=None):
        self.torch, self.kcap = torch, kcap
        nq = L["ids"].shape[0] if nq is None else nq
        self.ids = _dev(torch, L["ids"])
        self.dist = _dev(torch, L["dist"])
        self.k = _dev(torch, L["k"])
        self.labels = _dev(torch, L["labels"])
        self.skip = _dev(torch, L["skip"]) if skip else None
        self.truth = _dev(torch, L["truth"]) if truth else None
        shape = (L["ids"].shape[0], kcap)
        self.lab = RC.guarded(torch, shape, torch.int32)
        self.od = RC.guarded(torch, shape, torch.float64) if lists else None
        self.oi = RC.guarded(torch, shape, torch.int32) if lists else None
        self.hits = hits if hits is not None else \
            (RC.guarded(torch, kcap, torch.int64, fill=0) if truth else None)
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        g = lambda b: None if b is None else b.ptr()        # noqa: E731
        self.rc = _lib.lib().dmlp_vote_curve(
            p(self.dist) if lists else None, p(self.ids), L["ids"].shape[1], p(self.k), nq,
            p(self.skip), p(self.labels), kcap, g(self.lab), g(self.od), g(self.oi),
            p(self.truth), g(self.hits), _stream(torch))
        torch.cuda.synchronize()

    def check(self, ref, ctx, hits_times=1):
        assert self.rc == 0, ctx
        for b in (self.lab, self.od, self.oi, self.hits):
            if b is not None:
                b.check_guards(ctx)
        np.testing.assert_array_equal(self.lab.host(), ref[0], err_msg=f"{ctx}: labels")
        if self.oi is not None:
            np.testing.assert_array_equal(self.oi.host(), ref[2][1], err_msg=f"{ctx}: ids")
            np.testing.assert_array_equal(self.od.host(), ref[2][0], err_msg=f"{ctx}: dist")
        if self.hits is not None:
            np.testing.assert_array_equal(self.hits.host(), hits_times * ref[1],
                                          err_msg=f"{ctx}: hits")


SHAPES = [(kcap, ks) for kcap in KCAPS for ks in (kcap, kcap + 1, 300)]


@pytest.mark.parametrize("kcap,kstride", SHAPES)
def test_shapes(torch_cuda, kcap, kstride):
    """Every kcap at kstride = kcap, kcap + 1 and 300 (the clamp to 256 slots), nq on both sides of
    the four waves of a workgroup, the label space and the rotation of the rows moving along."""
    i = SHAPES.index((kcap, kstride))
    nq = (1, 3, 4, 5)[i % 4]
    space = SPACES[i % len(SPACES)]
    for seed in range(0, 7, 2):     # rows of other recipes / k / skip choices
        L, ref = VC.case(kcap, kstride, nq, space, seed)
        Run(torch_cuda, L, kcap).check(ref, f"kcap {kcap} kstride {kstride} nq {nq} seed {seed}")


@pytest.mark.parametrize("kcap,kstride,nq", [(33, 34, 257), (64, 300, 257), (256, 256, 43),
                                              (255, 300, 43), (2, 3, 8197)])
def test_many_rows(torch_cuda, kcap, kstride, nq):
    """257 rows: every (recipe, k, skip) combination, more than one workgroup; 8197 rows: past the
    2048 workgroups of the launch, so waves take more than one row and carry hits over them."""
    L, ref = VC.case(kcap, kstride, nq, "r513")
    Run(torch_cuda, L, kcap).check(ref, f"kcap {kcap} kstride {kstride} nq {nq}")


@pytest.mark.parametrize("space", SPACES)
def test_label_spaces(torch_cuda, space):
    L, ref = VC.case(64, 65, 42, space)
    Run(torch_cuda, L, 64).check(ref, space)
    assert 0 < ref[1].sum() < 42 * 64


@pytest.mark.parametrize("kcap,kstride", [(32, 33), (65, 300)])
def test_null_arguments(torch_cuda, kcap, kstride):
    """A null skip keeps every id >= 0; the list pair and the hits pair may each be left out (d may
    then be null as well), without a change to what is still written."""
    L, ref = VC.case(kcap, kstride, 42, "neg")
    L0, ref0 = VC.case(kcap, kstride, 42, "neg", with_skip=False)
    Run(torch_cuda, L0, kcap, skip=False).check(ref0, "null skip")
    Run(torch_cuda, L, kcap, lists=False).check(ref, "no lists")
    Run(torch_cuda, L, kcap, truth=False).check(ref, "no hits")
    Run(torch_cuda, L, kcap, truth=False, lists=False).check(ref, "labels only")
    assert (ref0[0] != ref[0]).any()


def test_hits_accumulate(torch_cuda):
    """hits is added to, like ovf_count: a second call into the same buffer doubles the counts,
    which are the column sums of the reference."""
    L, ref = VC.case(63, 64, 257, "two")
    first = Run(torch_cuda, L, 63)
    first.check(ref, "first call")
    Run(torch_cuda, L, 63, hits=first.hits).check(ref, "second call", hits_times=2)
    lab = ref[0]
    np.testing.assert_array_equal(ref[1], (lab == L["truth"][:, None]).sum(axis=0))


def test_argument_errors(torch_cuda):
    """-1 before any launch: kcap outside [1, 256], kstride < 1, a half-given pair; nq <= 0 returns
    0.  No output slot is written either way."""
    torch = torch_cuda
    Lb = _lib.lib()
    assert Lb.dmlp_vote_curve_kmax() == 256
    L, _ = VC.case(32, 33, 5, "ten")
    ids, dist, k = _dev(torch, L["ids"]), _dev(torch, L["dist"]), _dev(torch, L["k"])
    labels, truth = _dev(torch, L["labels"]), _dev(torch, L["truth"])
    lab = RC.guarded(torch, (5, 32), torch.int32)
    od = RC.guarded(torch, (5, 32), torch.float64)
    oi = RC.guarded(torch, (5, 32), torch.int32)
    hits = RC.guarded(torch, 32, torch.int64)

    def call(kstride=33, nq=5, kcap=32, o_d=od, o_i=oi, tr=truth, h=hits):
        g = lambda b: None if b is None else b.ptr()   # noqa: E731
        return Lb.dmlp_vote_curve(dist.data_ptr(), ids.data_ptr(), kstride, k.data_ptr(), nq, None,
                                  labels.data_ptr(), kcap, lab.ptr(), g(o_d), g(o_i),
                                  None if tr is None else tr.data_ptr(), g(h), _stream(torch))
    assert call(kcap=0) == -1 and call(kcap=257) == -1 and call(kcap=-3) == -1
    assert call(kstride=0) == -1
    assert call(o_d=None) == -1 and call(o_i=None) == -1
    assert call(tr=None) == -1 and call(h=None) == -1
    assert call(nq=0) == 0 and call(nq=-1) == 0
    torch.cuda.synchronize()
    for b in (lab, od, oi, hits):
        b.check_guards("argument errors")
        b.untouched(np.ones(b.t.shape, bool), "argument errors")


@pytest.mark.parametrize("space", ["ten", "extreme_lo", "r257"])
def test_finalize_is_the_oracle(torch_cuda, space):
    """dmlp_finalize, one launch per k, on the same device tensors: on the raw ids with a null skip
    (rows whose padding sits in the tail), and on the self-excluded list the curve kernel wrote."""
    torch = torch_cuda
    Lb = _lib.lib()
    kcap, kstride, nq = 64, 65, 42
    _, lo, hi = RC.label_space(space, VC.N_IDS, 0)
    L, ref = VC.case(kcap, kstride, nq, space)
    L0, ref0 = VC.case(kcap, kstride, nq, space, with_skip=False)
    run = Run(torch, L, kcap)
    run.check(ref, "skip")
    run0 = Run(torch, L0, kcap, skip=False)
    run0.check(ref0, "null skip")
    out = torch.empty(nq, dtype=torch.int32, device="cuda")
    cs = torch.empty(nq, dtype=torch.int64, device="cuda")
    rows = ~L["mid_negative"]

    def finalize(ids_ptr, stride, kq):
        kd = _dev(torch, kq.astype(np.int32))
        assert Lb.dmlp_finalize(None, ids_ptr, stride, kd.data_ptr(), None, nq,
                                run.labels.data_ptr(), lo, hi, out.data_ptr(), cs.data_ptr(),
                                _stream(torch)) == 0
        return out.cpu().numpy()
    got, got0 = run.lab.host(), run0.lab.host()
    for kk in (1, 2, 3, 4, 7, 31, 32, 33, 63, 64):
        lab = finalize(run.oi.ptr(), kcap, np.full(nq, kk))
        np.testing.assert_array_equal(lab, got[:, kk - 1], err_msg=f"compacted list, k={kk}")
        lab = finalize(run0.ids.data_ptr(), kstride, np.minimum(kk, np.clip(L["k"], 0, None)))
        np.testing.assert_array_equal(lab[rows], got0[rows, kk - 1], err_msg=f"raw list, k={kk}")
