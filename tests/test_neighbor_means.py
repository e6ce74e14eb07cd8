"""Kernel-level contract of the neighbour means (csrc/neighbor_means.hip, dmlp.h:
dmlp_neighbor_means / dmlp_neighbor_means_curve) through the C ABI.

Every output goes into a buffer of exactly its size between sentinel bands
(tests/helpers/result_contract.py: guarded) and every slot is compared with the plain-Python
reference of tests/helpers/neighbor_means_contract.py (pinned against the CPU twins by
tests/test_neighbor_means_model.py): means and weight sums on their bits, NaN where the contract
says NaN, counts as integers.

The lists are vote_curve_contract's rotation of row recipes, k choices and skips, followed by the
special rows of neighbor_means_contract (order-sensitive sums at the start, in the middle, across
the slot-256 boundary and behind 255 dropped entries, a contraction-sensitive product, zero, +inf,
subnormal and huge distances, an overflowing sum, an empty row)."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import neighbor_means_contract as NM  # noqa: E402
import result_contract as RC  # noqa: E402

pytestmark = pytest.mark.gpu

KSTRIDES = (1, 7, 64, 255, 256, 257, 300, 600)   # chunk boundaries, a second and a third chunk
TS = (1, 2, 3, 63, 64, 65, 130, 256)             # lane passes
KCAPS = (1, 31, 33, 63, 65, 255, 256, 64)        # both sides of 32, 64 and 256
BLOCKS = 2048                                    # workgroups of a launch, four rows each


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
    """One dmlp_neighbor_means and one dmlp_neighbor_means_curve call into guarded outputs."""

    def __init__(self, torch, L, mode, kcap, skip=True, dist=True, wsum=True, count=True):
        nq, ks = L["ids"].shape
        T = L["targets"].shape[1]
        self.ids = _dev(torch, L["ids"])
        self.dist = _dev(torch, L["dist"]) if dist else None
        self.k = _dev(torch, L["k"])
        self.targets = _dev(torch, L["targets"])
        self.skip = _dev(torch, L["skip"]) if skip else None
        self.mean = RC.guarded(torch, (nq, T), torch.float64)
        self.wsum = RC.guarded(torch, nq, torch.float64) if wsum else None
        self.count = RC.guarded(torch, nq, torch.int32) if count else None
        self.curve = RC.guarded(torch, (nq, kcap, T), torch.float64)
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        g = lambda b: None if b is None else b.ptr()        # noqa: E731
        Lb = _lib.lib()
        self.rc = Lb.dmlp_neighbor_means(
            p(self.dist), p(self.ids), ks, p(self.k), nq, p(self.skip), p(self.targets), T, mode,
            g(self.mean), g(self.wsum), g(self.count), _stream(torch))
        self.rc_curve = Lb.dmlp_neighbor_means_curve(
            p(self.dist), p(self.ids), ks, p(self.k), nq, p(self.skip), p(self.targets), T, mode,
            kcap, g(self.curve), _stream(torch))
        torch.cuda.synchronize()

    def check(self, ref, ctx):
        assert self.rc == 0 and self.rc_curve == 0, ctx
        for b in (self.mean, self.wsum, self.count, self.curve):
            if b is not None:
                b.check_guards(ctx)
        NM.assert_same(self.mean.host(), ref[0], f"{ctx}: mean")
        if self.wsum is not None:
            NM.assert_same(self.wsum.host(), ref[1], f"{ctx}: wsum")
        if self.count is not None:
            np.testing.assert_array_equal(self.count.host(), ref[2], err_msg=f"{ctx}: count")
        NM.assert_same(self.curve.host(), ref[3], f"{ctx}: curve")


SHAPES = [(ks, TS[(i + j) % 8], KCAPS[(i + 2 * j) % 8])
          for i, ks in enumerate(KSTRIDES) for j in (0, 3, 6)]


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("kstride,T,kcap", SHAPES)
def test_shapes(torch_cuda, kstride, T, kcap, mode):
    """Every kstride with three target counts and three kcaps (each T with three strides), nq on
    both sides of the four waves of a workgroup."""
    i = SHAPES.index((kstride, T, kcap))
    nq = (1, 3, 4, 5)[i % 4]
    L, ref = NM.case(kcap, kstride, nq, T, mode, seed=i % 7)
    Run(torch_cuda, L, mode, kcap).check(ref, f"kstride {kstride} T {T} kcap {kcap} nq {nq} "
                                              f"mode {mode}")


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("kstride,T,kcap", [(64, 1, 32), (300, 3, 256), (600, 65, 100)])
def test_many_rows(torch_cuda, kstride, T, kcap, mode):
    """37 rows and the special ones: more than one workgroup, most (recipe, k, skip) combinations."""
    L, ref = NM.case(kcap, kstride, 37, T, mode, seed=1)
    Run(torch_cuda, L, mode, kcap).check(ref, f"kstride {kstride} T {T} kcap {kcap} mode {mode}")


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("kstride,kcap", [(7, 5), (255, 63), (256, 256), (300, 255), (600, 65),
                                          (600, 129)])
def test_single_target(torch_cuda, kstride, kcap, mode):
    """T == 1 takes a kernel of its own (the gather rides on the compaction, a lane keeps the
    running sums of its curve slots): one, two and three chunks, kcap on both sides of its 64-slot
    groups."""
    L, ref = NM.case(kcap, kstride, 37, 1, mode, seed=3)
    Run(torch_cuda, L, mode, kcap).check(ref, f"kstride {kstride} kcap {kcap} mode {mode}")


@pytest.mark.parametrize("mode", (0, 1))
def test_rows_past_the_grid(torch_cuda, mode):
    """Just past the launch's 2048 workgroups of four rows: waves take a second row."""
    L, ref = NM.case(2, 3, 4 * BLOCKS + 5, 1, mode)
    Run(torch_cuda, L, mode, 2).check(ref, f"mode {mode}")


@pytest.mark.parametrize("mode", (0, 1))
def test_null_arguments(torch_cuda, mode):
    """A null skip keeps every id >= 0; out_wsum and out_count may each be left out without a
    change to what is still written; mode 0 reads no distance."""
    L, ref = NM.case(40, 300, 37, 3, mode, seed=2)
    L0, ref0 = NM.case(40, 300, 37, 3, mode, seed=2, with_skip=False)
    Run(torch_cuda, L0, mode, 40, skip=False).check(ref0, "null skip")
    assert (ref0[2] != ref[2]).any()
    Run(torch_cuda, L, mode, 40, wsum=False).check(ref, "no wsum")
    Run(torch_cuda, L, mode, 40, count=False).check(ref, "no count")
    Run(torch_cuda, L, mode, 40, wsum=False, count=False).check(ref, "means only")
    if mode == 0:
        Run(torch_cuda, L, 0, 40, dist=False).check(ref, "null d")


def test_argument_errors(torch_cuda):
    """-1 before any launch: T outside [1, tmax], kstride < 1, a mode that is neither 0 nor 1, mode
    1 without d, kcap outside [1, 256], a null out_mean, ids, qk or targets; nq <= 0 returns 0.  No
    output slot is written either way."""
    torch = torch_cuda
    Lb = _lib.lib()
    assert Lb.dmlp_neighbor_means_tmax() == NM.TMAX
    L, _ = NM.case(5, 7, 5, 3, 1)
    nq = L["ids"].shape[0]
    ids, dist, k = _dev(torch, L["ids"]), _dev(torch, L["dist"]), _dev(torch, L["k"])
    tg = _dev(torch, L["targets"])
    mean = RC.guarded(torch, (nq, 5, 3), torch.float64)
    wsum = RC.guarded(torch, nq, torch.float64)
    count = RC.guarded(torch, nq, torch.int32)
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731

    def means(kstride=7, n=nq, T=3, mode=1, d=dist, i=ids, kk=k, t=tg, o=mean.ptr()):
        return Lb.dmlp_neighbor_means(p(d), p(i), kstride, p(kk), n, None, p(t), T, mode, o,
                                      wsum.ptr(), count.ptr(), _stream(torch))

    def curve(kstride=7, n=nq, T=3, mode=1, kcap=5, d=dist, i=ids, kk=k, t=tg, o=mean.ptr()):
        return Lb.dmlp_neighbor_means_curve(p(d), p(i), kstride, p(kk), n, None, p(t), T, mode,
                                            kcap, o, _stream(torch))
    for call in (means, curve):
        assert call(T=0) == -1 and call(T=NM.TMAX + 1) == -1 and call(T=-1) == -1
        assert call(kstride=0) == -1
        assert call(mode=2) == -1 and call(mode=-1) == -1
        assert call(d=None) == -1
        assert call(i=None) == -1 and call(kk=None) == -1 and call(t=None) == -1
        assert call(o=None) == -1
        assert call(n=0) == 0 and call(n=-1) == 0
    assert curve(kcap=0) == -1 and curve(kcap=257) == -1 and curve(kcap=-3) == -1
    torch.cuda.synchronize()
    for b in (mean, wsum, count):
        b.check_guards("argument errors")
        b.untouched(np.ones(b.t.shape, bool), "argument errors")
