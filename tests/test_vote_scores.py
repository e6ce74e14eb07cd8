"""Kernel-level contract of the class scores (csrc/vote_scores.hip, dmlp.h: dmlp_vote_scores) through
the C ABI.

Every output goes into a buffer of exactly nq * nclass / nq slots between sentinel bands
(tests/helpers/result_contract.py: guarded) and every slot is compared with the plain-Python
reference of tests/helpers/vote_scores_contract.py (pinned against the CPU twin by
tests/test_vote_scores_model.py): counts and labels as integers, scores on their bits.
dmlp_finalize over the same device lists is the second oracle of mode 0's label.

The lists are vote_curve_contract's rotation of row recipes, k choices and skips, followed by the
special rows of vote_scores_contract (order-sensitive sums at the start, in the middle and across
the 256-slot chunk boundary, +inf and subnormal weights, ties, labels outside the class range)."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import result_contract as RC  # noqa: E402
import vote_scores_contract as VS  # noqa: E402

pytestmark = pytest.mark.gpu

KSTRIDES = (1, 7, 64, 255, 256, 257, 300, 600)       # chunk boundaries, a second and a third chunk
NCLASSES = (1, 2, 63, 64, 65, 130, 300, VS.CMAX)     # lane passes
LABEL_LOS = (-3, 0, -64, 41, -100, -1, -150, -2048)
BLOCKS = 2048                                        # workgroups of a launch, four rows each
CMAX_ROWS = ("order", "order_chunk", "inf_label", "tie", "nothing")


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
    """One dmlp_vote_scores call into guarded outputs."""

    def __init__(self, torch, L, mode, skip=True, dist=True, count=True, score=True, label=True):
        self.torch = torch
        nq, ks = L["ids"].shape
        nclass = L["nclass"]
        self.ids = _dev(torch, L["ids"])
        self.dist = _dev(torch, L["dist"]) if dist else None
        self.k = _dev(torch, L["k"])
        self.labels = _dev(torch, L["labels"])
        self.skip = _dev(torch, L["skip"]) if skip else None
        self.cnt = RC.guarded(torch, (nq, nclass), torch.int32) if count else None
        self.sc = RC.guarded(torch, (nq, nclass), torch.float64) if score else None
        self.lab = RC.guarded(torch, nq, torch.int32) if label else None
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        g = lambda b: None if b is None else b.ptr()        # noqa: E731
        self.rc = _lib.lib().dmlp_vote_scores(
            p(self.dist), p(self.ids), ks, p(self.k), nq, p(self.skip), p(self.labels),
            L["label_lo"], nclass, mode, g(self.cnt), g(self.sc), g(self.lab), _stream(torch))
        torch.cuda.synchronize()

    def check(self, ref, ctx):
        assert self.rc == 0, ctx
        for b in (self.cnt, self.sc, self.lab):
            if b is not None:
                b.check_guards(ctx)
        if self.cnt is not None:
            np.testing.assert_array_equal(self.cnt.host(), ref[0], err_msg=f"{ctx}: count")
        if self.sc is not None:
            np.testing.assert_array_equal(self.sc.host().view(np.int64), ref[1].view(np.int64),
                                          err_msg=f"{ctx}: score bits")
        if self.lab is not None:
            np.testing.assert_array_equal(self.lab.host(), ref[2], err_msg=f"{ctx}: label")


SHAPES = [(ks, NCLASSES[(i + j) % 8], LABEL_LOS[(i + j) % 8])
          for i, ks in enumerate(KSTRIDES) for j in (0, 3, 6)]


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("kstride,nclass,label_lo", SHAPES)
def test_shapes(torch_cuda, kstride, nclass, label_lo, mode):
    """Every kstride with three class counts (each class count with three strides), nq on both
    sides of the four waves of a workgroup, labels below and above the class range."""
    i = SHAPES.index((kstride, nclass, label_lo))
    nq = (1, 3, 4, 5)[i % 4]
    only = None
    if nclass == VS.CMAX:   # at most 8 rows of 4096 classes: three rotated rows, five special ones
        nq, only = 3, CMAX_ROWS
    L, ref = VS.case(kstride, nq, "ten", i % 7, nclass, label_lo, mode, only=only)
    assert nclass < VS.CMAX or L["ids"].shape[0] <= 8
    Run(torch_cuda, L, mode).check(ref, f"kstride {kstride} nclass {nclass} nq {nq} mode {mode}")


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("kstride,nclass,label_lo", [(64, 10, -4), (300, 130, -100), (600, 65, 0)])
def test_many_rows(torch_cuda, kstride, nclass, label_lo, mode):
    """37 rows and the special ones: more than one workgroup, most (recipe, k, skip) combinations."""
    L, ref = VS.case(kstride, 37, "ten", 1, nclass, label_lo, mode)
    Run(torch_cuda, L, mode).check(ref, f"kstride {kstride} nclass {nclass} mode {mode}")


@pytest.mark.parametrize("mode", (0, 1))
def test_rows_past_the_grid(torch_cuda, mode):
    """Just past the launch's 2048 workgroups of four rows: waves take a second row."""
    L, ref = VS.case(4, 4 * BLOCKS + 5, "ten", 0, 3, -1, mode)
    Run(torch_cuda, L, mode).check(ref, f"mode {mode}")


@pytest.mark.parametrize("space", [s for s in RC.LABEL_SPACES if not s.startswith("extreme")])
def test_label_spaces(torch_cuda, space):
    """The label spaces whose range fits, with the range they state (the labels' own for
    "unknown")."""
    for mode in (0, 1):
        L, ref = VS.case(65, 42, space, mode=mode)
        Run(torch_cuda, L, mode).check(ref, f"{space} mode {mode}")


@pytest.mark.parametrize("mode", (0, 1))
def test_null_arguments(torch_cuda, mode):
    """A null skip keeps every id >= 0; each output may be left out without a change to what is
    still written; mode 0 reads no distance."""
    L, ref = VS.case(300, 37, "ten", 2, 65, -30, mode)
    L0, ref0 = VS.case(300, 37, "ten", 2, 65, -30, mode, with_skip=False)
    Run(torch_cuda, L0, mode, skip=False).check(ref0, "null skip")
    assert (ref0[0] != ref[0]).any()
    Run(torch_cuda, L, mode, count=False).check(ref, "no count")
    Run(torch_cuda, L, mode, score=False).check(ref, "no score")
    Run(torch_cuda, L, mode, label=False).check(ref, "no label")
    Run(torch_cuda, L, mode, count=False, score=False).check(ref, "label only")
    if mode == 0:
        Run(torch_cuda, L, 0, dist=False).check(ref, "null d")


def test_argument_errors(torch_cuda):
    """-1 before any launch: nclass outside [1, cmax], kstride < 1, a mode that is neither 0 nor 1,
    mode 1 without d, no output at all; nq <= 0 returns 0.  No output slot is written either way."""
    torch = torch_cuda
    Lb = _lib.lib()
    assert Lb.dmlp_vote_scores_cmax() == VS.CMAX
    L, _ = VS.case(7, 5, "ten", 0, 3, -1, 1)
    nq = L["ids"].shape[0]
    ids, dist, k = _dev(torch, L["ids"]), _dev(torch, L["dist"]), _dev(torch, L["k"])
    labels = _dev(torch, L["labels"])
    cnt = RC.guarded(torch, (nq, 3), torch.int32)
    sc = RC.guarded(torch, (nq, 3), torch.float64)
    lab = RC.guarded(torch, nq, torch.int32)

    def call(kstride=7, n=nq, nclass=3, mode=1, d=dist, oc=cnt, os_=sc, ol=lab):
        g = lambda b: None if b is None else b.ptr()   # noqa: E731
        return Lb.dmlp_vote_scores(None if d is None else d.data_ptr(), ids.data_ptr(), kstride,
                                   k.data_ptr(), n, None, labels.data_ptr(), -1, nclass, mode,
                                   g(oc), g(os_), g(ol), _stream(torch))
    assert call(nclass=0) == -1 and call(nclass=VS.CMAX + 1) == -1 and call(nclass=-2) == -1
    assert call(kstride=0) == -1
    assert call(mode=2) == -1 and call(mode=-1) == -1
    assert call(d=None) == -1
    assert call(oc=None, os_=None, ol=None) == -1
    assert call(n=0) == 0 and call(n=-1) == 0
    torch.cuda.synchronize()
    for b in (cnt, sc, lab):
        b.check_guards("argument errors")
        b.untouched(np.ones(b.t.shape, bool), "argument errors")


@pytest.mark.parametrize("space", ["ten", "r257", "neg"])
def test_finalize_is_the_oracle(torch_cuda, space):
    """dmlp_finalize on the same device lists (null skip: finalize has none; k clamped to the
    stride, which finalize does not do itself): mode 0's label is its vote."""
    torch = torch_cuda
    Lb = _lib.lib()
    for kstride in (65, 300):
        L, ref = VS.case(kstride, 42, space, mode=0, with_skip=False)
        run = Run(torch, L, 0, skip=False)
        run.check(ref, f"{space} kstride {kstride}")
        nq = L["ids"].shape[0]
        labels, lo, hi = RC.label_space(space, VS.N_IDS)
        out = torch.empty(nq, dtype=torch.int32, device="cuda")
        cs = torch.empty(nq, dtype=torch.int64, device="cuda")
        kd = _dev(torch, np.clip(L["k"], 0, kstride).astype(np.int32))
        assert Lb.dmlp_finalize(None, run.ids.data_ptr(), kstride, kd.data_ptr(), None, nq,
                                run.labels.data_ptr(), lo, hi, out.data_ptr(), cs.data_ptr(),
                                _stream(torch)) == 0
        np.testing.assert_array_equal(run.lab.host(), out.cpu().numpy(),
                                      err_msg=f"{space} kstride {kstride}")
