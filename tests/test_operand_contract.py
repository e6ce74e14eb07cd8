"""Kernel-level contract of the operand prep, the int32 row transfer and the point-major copy
(prep.hip; the copy: k_x1_rowmajor), through the C ABI.

End-to-end runs reach these kernels on uniform six-decimal data only, where the later stages
repair or hide a wrong bit.  Here every entry point is called directly into outputs with
sentinel bands around them (tests/helpers/result_contract.py: guarded) and every 16-bit word,
float and flag is compared with the NumPy references of tests/helpers/operand_contract.py
(pinned on the CPU by tests/test_operand_contract_model.py).  All comparisons are bit-exact but
three derived bounds:
  xinit / qn of the bf16 prep   within one fp32 step of the correctly rounded |c|^2 (the kernel's
                                fp64 sum of <= 256 non-negative terms is off by < 258 * 2^-53
                                relative, so only the final fp32 rounding can differ)
  its max norm m                fp32(max |c|^2) <= m <= max |c|^2 (1 + 3e-6)
  dmlp_center                   |mu - mean| <= (n + 1) 2^-53 sum|x| / n (any order, one division)
"""
import functools
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import operand_contract as OC  # noqa: E402
import result_contract as RC  # noqa: E402

pytestmark = pytest.mark.gpu


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
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u16(g):
    """the payload of a guarded uint8 buffer as uint16"""
    return g.host().view(np.uint16)


class Words:
    """Guarded uint32 words (an int32 buffer) with preset values."""

    def __init__(self, torch, values):
        self.g = RC.guarded(torch, len(values), torch.int32, fill=0)
        self.g.t.copy_(torch.from_numpy(np.array(values, np.uint32).view(np.int32)))

    def ptr(self, i=0):
        return self.g.ptr() + 4 * i

    def get(self, ctx=""):
        self.g.check_guards(ctx + " words")
        return self.g.host().view(np.uint32)


F32 = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731


# ------------------------------------------------------------------ dmlp_prep_data / _queries
PREP_CASES = [(1, 1), (7, 1), (32, 1), (33, 2), (64, 2), (100, 4), (256, 8), (70, 3)]
PREP_N = (1, 63, 64, 65, 130)
PREP_Q = (1, 63, 65)


@functools.lru_cache(maxsize=None)
def prep_input(n, A, seed):
    mu = OC.prep_mu(A)
    return OC.prep_rows(n, A, mu, seed), mu


def check_norms(got, want64, ctx):
    ok = OC.within_one_ulp32(got, want64)
    assert ok.all(), f"{ctx}: rows {np.flatnonzero(~ok)[:4].tolist()} off by more than one fp32 step"


def run_prep_data(torch, X, mu, KT, ctx, expect_bad):
    L = _lib.lib()
    N, A = X.shape
    nt = (N + 63) // 64
    ref, c, bad = OC.hilo_image(X, mu, KT)
    assert bad == expect_bad, ctx
    dX, dmu = _dev(torch, X), _dev(torch, mu)
    img = RC.guarded(torch, nt * 64 * KT * 64 * 2, torch.uint8)
    xin = RC.guarded(torch, nt * 64, torch.float32)
    small = 2.0 ** -100                           # below every norm of these inputs
    w = Words(torch, [F32(small), 2])             # xnmax_bits, bad: preset, must accumulate
    args = (dX.data_ptr(), N, A, dmu.data_ptr(), KT, img.ptr(), xin.ptr())
    assert L.dmlp_prep_data(*args, w.ptr(0), w.ptr(1), _stream(torch)) == 0, ctx
    img.check_guards(ctx + " image")
    xin.check_guards(ctx + " xinit")
    np.testing.assert_array_equal(u16(img), ref, err_msg=ctx + " image")
    x = xin.host()
    assert np.isneginf(x[N:]).all(), f"{ctx}: xinit of the padding rows"
    ss = OC.norms_exact(c)
    check_norms(x[:N], -0.5 * ss, ctx + " xinit")
    m_bits, b = w.get(ctx)
    assert b == (2 | expect_bad), f"{ctx}: bad {b}"
    m = float(np.uint32(m_bits).view(np.float32))
    smax = float(ss.max())
    assert smax > 1.0, ctx                        # (the + 1e-30 of the kernel is far below it)
    assert float(np.float32(smax)) <= m <= smax * (1 + 3e-6), f"{ctx}: max norm {m} of {smax}"
    # a larger preset stays: the max norm is max-ed into the word
    w2 = Words(torch, [0x7f000000, 0])
    assert L.dmlp_prep_data(*args, w2.ptr(0), w2.ptr(1), _stream(torch)) == 0, ctx
    m2, b2 = w2.get(ctx)
    assert m2 == 0x7f000000 and b2 == expect_bad, f"{ctx}: presets ({m2:#x}, {b2})"


def run_prep_queries(torch, Qx, mu, KT, ctx, expect_bad):
    L = _lib.lib()
    Q, A = Qx.shape
    W = KT * 32
    rhi, rlo, c, bad = OC.query_frags(Qx, mu, KT)
    assert bad == expect_bad, ctx
    dQ, dmu = _dev(torch, Qx), _dev(torch, mu)
    qhi = RC.guarded(torch, Q * W * 2, torch.uint8)
    qlo = RC.guarded(torch, Q * W * 2, torch.uint8)
    qn = RC.guarded(torch, Q, torch.float32)
    w = Words(torch, [4])
    assert L.dmlp_prep_queries(dQ.data_ptr(), Q, A, dmu.data_ptr(), KT, qhi.ptr(), qlo.ptr(),
                               qn.ptr(), w.ptr(0), _stream(torch)) == 0, ctx
    for g, name in ((qhi, "qhi"), (qlo, "qlo"), (qn, "qn")):
        g.check_guards(f"{ctx} {name}")
    np.testing.assert_array_equal(u16(qhi).reshape(Q, W), rhi, err_msg=ctx + " qhi")
    np.testing.assert_array_equal(u16(qlo).reshape(Q, W), rlo, err_msg=ctx + " qlo")
    check_norms(qn.host(), OC.norms_exact(c), ctx + " qn")
    assert w.get(ctx)[0] == (4 | expect_bad), f"{ctx}: bad"


def flagged(X, mu):
    """(value, row, attribute, copy of X with that element out of range) over the flag set, each
    in the first row, the last row and the last attribute"""
    n, A = X.shape
    for v in OC.BF16_FLAGS:
        for r, a in ((0, 0), (n - 1, 0), (n // 2, A - 1)):
            assert mu[a] == 0.0
            Y = X.copy()
            Y[r, a] = v
            yield v, r, a, Y


@pytest.mark.parametrize("A,KT", PREP_CASES)
def test_prep_data_contract(torch_cuda, A, KT):
    """Every uint16 of the hi/lo image (padding rows and columns included), xinit, the max norm
    and the accumulating words, for every N around the tile and every kernel behind the entry
    point (KT 3: k_prep_frag + k_prep_norm)."""
    for N in PREP_N:
        X, mu = prep_input(N, A, 0)
        run_prep_data(torch_cuda, X, mu, KT, f"prep_data A={A} KT={KT} N={N}", 0)
    X, mu = prep_input(65, A, 0)
    for v, r, a, Y in flagged(X, mu):
        run_prep_data(torch_cuda, Y, mu, KT, f"prep_data A={A} KT={KT} {v} at ({r}, {a})", 1)


@pytest.mark.parametrize("A,KT", PREP_CASES)
def test_prep_queries_contract(torch_cuda, A, KT):
    """qhi = bf16(c), qlo = bf16(c - hi) bit for bit, zero padding columns, qn, bad (KT 3:
    k_prep_queries)."""
    for Q in PREP_Q:
        Qx, mu = prep_input(Q, A, 1)
        run_prep_queries(torch_cuda, Qx, mu, KT, f"prep_queries A={A} KT={KT} Q={Q}", 0)
    Qx, mu = prep_input(65, A, 1)
    for v, r, a, Y in flagged(Qx, mu):
        run_prep_queries(torch_cuda, Y, mu, KT, f"prep_queries A={A} KT={KT} {v} at ({r}, {a})", 1)


def test_prep_rejects_bad_shapes(torch_cuda):
    """KT < 1 and A > 32 KT return -1 and write nothing."""
    torch = torch_cuda
    L = _lib.lib()
    X, mu = prep_input(65, 33, 0)
    dX, dmu = _dev(torch, X), _dev(torch, mu)
    for KT in (0, -1, 1):
        img = RC.guarded(torch, 128 * 2 * 64 * 2, torch.uint8)
        lo = RC.guarded(torch, 128 * 2 * 64 * 2, torch.uint8)
        xin = RC.guarded(torch, 128, torch.float32)
        w = Words(torch, [5, 6])
        assert L.dmlp_prep_data(dX.data_ptr(), 65, 33, dmu.data_ptr(), KT, img.ptr(), xin.ptr(),
                                w.ptr(0), w.ptr(1), _stream(torch)) == -1
        assert L.dmlp_prep_queries(dX.data_ptr(), 65, 33, dmu.data_ptr(), KT, img.ptr(), lo.ptr(),
                                   xin.ptr(), w.ptr(1), _stream(torch)) == -1
        for g in (img, lo, xin):
            g.check_guards(f"KT={KT}")
            g.untouched(np.ones(g.n, bool), f"KT={KT}")
        assert list(w.get()) == [5, 6]


# ------------------------------------------------------------------ dmlp_render_rows
def kt_of(A):
    return 1 if A <= 32 else 2 if A <= 64 else 4 if A <= 128 else 8


class Render:
    """One set of guarded outputs of dmlp_render_rows for rows [0, n_pad) x W."""

    def __init__(self, torch, n_pad, nsrc, A, KT, mode):
        W = KT * 32
        self.torch, self.A, self.KT, self.mode = torch, A, KT, mode
        self.img = RC.guarded(torch, n_pad * W * 2, torch.uint8)
        self.xq = RC.guarded(torch, n_pad, torch.float32)
        self.xrow = RC.guarded(torch, n_pad * W * 2, torch.uint8)
        self.dst = RC.guarded(torch, max(nsrc, 1) * A, torch.float64)
        self.w = Words(torch, [0, 0, 0, 0])     # nmax, bad, done, rdy

    def call(self, src, i32, r0, n, nvalid, mu, null=False):
        L = _lib.lib()
        w = self.w
        s = (src.data_ptr(), None) if i32 else (None, src.data_ptr())
        # xrow, nmax, bad, done, rdy (null: none of them, nor dst64)
        opt = [None] * 5 if null else [self.xrow.ptr() if self.mode == 0 else None, w.ptr(0),
                                       w.ptr(1), w.ptr(2), w.ptr(3)]
        dst = None if null else self.dst.ptr()
        return L.dmlp_render_rows(self.KT, self.A, *s, r0, n, nvalid, mu.data_ptr(), dst,
                                  self.mode, self.img.ptr(), self.xq.ptr(), *opt,
                                  _stream(self.torch))

    def guards(self, ctx):
        for g, name in ((self.img, "img"), (self.xq, "xq"), (self.xrow, "xrow"),
                        (self.dst, "dst64")):
            g.check_guards(f"{ctx} {name}")


def host_render(X, mu, KT, mode):
    """host_prep.cpp's render of the same rows: (img, xq, nmax bits or None)"""
    L = _lib.lib()
    n, A = X.shape
    W = KT * 32
    if mode == 1:
        hh = np.zeros((n, W), np.uint16)
        qn = np.zeros(n, np.float32)
        assert L.dmlp_cpu_prep_queries(X.ctypes.data, n, A, mu.ctypes.data, KT, hh.ctypes.data,
                                       qn.ctypes.data) == 0
        return hh, qn, None
    nt = (n + 63) // 64
    img = np.zeros(nt * 64 * W, np.uint16)
    xin = np.zeros(nt * 64, np.float32)
    nm = np.zeros(1, np.uint32)
    assert L.dmlp_cpu_prep_data(X.ctypes.data, n, A, mu.ctypes.data, KT, img.ctypes.data,
                                xin.ctypes.data, nm.ctypes.data) == 0
    return img, xin, int(nm[0])


def eq_bits(a, b, msg):
    np.testing.assert_array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32),
                                  err_msg=msg)


@pytest.mark.parametrize("i32", [False, True], ids=["f64", "i32"])
@pytest.mark.parametrize("A", [7, 32, 40, 100, 200])
def test_render_dataset_contract(torch_cuda, A, i32):
    """Mode 0 on the fp16 edge set (fp64 rows) and on int32 rows over the whole int32 range: two
    slices (the second with r0 > 0) whose max norms accumulate, nvalid inside the last tile; image,
    xinit, -inf padding, xrow, *nmax, dst64 against render_model and against the host render; the
    ready word per call; then the same image with every optional pointer null."""
    torch = torch_cuda
    KT, N = kt_of(A), 130
    W = KT * 32
    X, mu, m = OC.render_rows(N, A, i32=i32)
    ref = OC.render_model(X, mu, KT, 0)
    assert ref["bad"] == 0
    src = _dev(torch, m.reshape(-1) if i32 else X.reshape(-1))
    dmu = _dev(torch, mu)
    ctx = f"render rows A={A} {'i32' if i32 else 'f64'}"
    R = Render(torch, 192, N, A, KT, 0)
    run_max = 0
    for j, (r0, n) in enumerate(((0, 64), (64, 128))):
        if j:
            R.w.g.t[2:] = 0                           # done / rdy: zeroed by the caller per call
        assert R.call(src, i32, r0, n, N, dmu) == 0, ctx
        run_max = max(run_max, OC.nmax_bits(ref["up"][r0:min(N, r0 + n)]))
        w = R.w.get(ctx)
        assert w[0] == run_max, f"{ctx}: *nmax after slice {j}"
        assert w[1] == 0 and w[2] == n // 64 and w[3] == 1, f"{ctx}: words {w.tolist()} slice {j}"
    R.guards(ctx)
    np.testing.assert_array_equal(u16(R.img), ref["img"], err_msg=ctx + " image")
    eq_bits(R.xq.host(), ref["xq"], ctx + " xinit")
    assert np.isneginf(R.xq.host()[N:]).all()
    np.testing.assert_array_equal(u16(R.xrow).reshape(192, W), ref["xrow"], err_msg=ctx + " xrow")
    if i32:
        np.testing.assert_array_equal(R.dst.host().view(np.uint64),
                                      X.reshape(-1).view(np.uint64), err_msg=ctx + " dst64")
    else:
        R.dst.untouched(np.ones(N * A, bool), ctx + " dst64 (fp64 source)")
    himg, hxin, hnm = host_render(X, mu, KT, 0)
    np.testing.assert_array_equal(u16(R.img), himg, err_msg=ctx + " image vs host")
    eq_bits(R.xq.host(), hxin, ctx + " xinit vs host")
    assert run_max == hnm, f"{ctx}: max norm vs host"
    # every optional pointer null: the same image and xinit, nothing else
    R2 = Render(torch, 192, N, A, KT, 0)
    assert R2.call(src, i32, 0, 192, N, dmu, null=True) == 0
    R2.guards(ctx + " null")
    np.testing.assert_array_equal(u16(R2.img), ref["img"], err_msg=ctx + " image (null)")
    eq_bits(R2.xq.host(), ref["xq"], ctx + " xinit (null)")
    R2.xrow.untouched(np.ones(R2.xrow.n, bool), ctx + " xrow (null)")
    R2.dst.untouched(np.ones(R2.dst.n, bool), ctx + " dst64 (null)")
    assert list(R2.w.get()) == [0, 0, 0, 0]


@pytest.mark.parametrize("i32", [False, True], ids=["f64", "i32"])
@pytest.mark.parametrize("A", [7, 32, 40, 100, 200])
def test_render_queries_contract(torch_cuda, A, i32):
    """Mode 1 for Q in {1, 63, 65} and as two blocks (the second with r0 > 0): qhi, qn, dst64
    against render_model and the host; rows past the block untouched."""
    torch = torch_cuda
    KT = kt_of(A)
    W = KT * 32
    for Q, blocks in ((1, ((0, 1),)), (63, ((0, 63),)), (65, ((0, 65),)), (65, ((0, 30), (30, 35)))):
        X, mu, m = OC.render_rows(Q, A, seed=5, i32=i32)
        ref = OC.render_model(X, mu, KT, 1)
        src = _dev(torch, m.reshape(-1) if i32 else X.reshape(-1))
        dmu = _dev(torch, mu)
        ctx = f"render queries A={A} Q={Q} {blocks} {'i32' if i32 else 'f64'}"
        R = Render(torch, Q + 3, Q, A, KT, 1)
        for r0, n in blocks:
            R.w.g.t[2:] = 0
            assert R.call(src, i32, r0, n, Q, dmu) == 0, ctx
            w = R.w.get(ctx)
            assert w[0] == 0 and w[1] == 0 and w[2] == (n + 63) // 64 and w[3] == 1, \
                f"{ctx}: words {w.tolist()}"
        R.guards(ctx)
        np.testing.assert_array_equal(u16(R.img).reshape(Q + 3, W)[:Q], ref["img"], err_msg=ctx)
        eq_bits(R.xq.host()[:Q], ref["xq"], ctx + " qn")
        keep = np.zeros((Q + 3, W * 2), bool)
        keep[Q:] = True
        R.img.untouched(keep.reshape(-1), ctx + " qhi past Q")
        R.xq.untouched(np.arange(Q + 3) >= Q, ctx + " qn past Q")
        if i32:
            np.testing.assert_array_equal(R.dst.host().view(np.uint64),
                                          X.reshape(-1).view(np.uint64), err_msg=ctx + " dst64")
        hh, hqn, _ = host_render(X, mu, KT, 1)
        np.testing.assert_array_equal(u16(R.img).reshape(Q + 3, W)[:Q], hh, err_msg=ctx + " host")
        eq_bits(R.xq.host()[:Q], hqn, ctx + " qn vs host")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("A", [7, 40])
def test_render_flags(torch_cuda, A, mode):
    """+-65504 (and 1e6, inf, NaN) in an fp64 row — a dataset row or a query row — sets *bad (OR-ed
    into its value) and renders as 0, left out of the norm; +-65503.99 does not."""
    torch = torch_cuda
    KT, n = kt_of(A), 64
    X, mu, _ = OC.render_rows(n, A, seed=2)
    dmu = _dev(torch, mu)
    for v in (*OC.FP16_FLAGS, 65503.99, -65503.99):
        for r, a in ((0, 0), (n - 1, 0), (n // 2, A - 1)):
            Y = X.copy()
            Y[r, a] = v + mu[a]
            ref = OC.render_model(Y, mu, KT, mode)
            assert ref["bad"] == (abs(v) < 65504.0) ^ 1
            ctx = f"render flag A={A} mode={mode} {v} at ({r}, {a})"
            R = Render(torch, n, n, A, KT, mode)
            R.w = Words(torch, [0, 2, 0, 0])
            assert R.call(_dev(torch, Y.reshape(-1)), False, 0, n, n, dmu) == 0, ctx
            R.guards(ctx)
            assert R.w.get(ctx)[1] == (2 | ref["bad"]), ctx
            np.testing.assert_array_equal(u16(R.img), ref["img"].reshape(-1), err_msg=ctx)
            eq_bits(R.xq.host(), ref["xq"], ctx)
            if mode == 0:
                assert R.w.get()[0] == OC.nmax_bits(ref["up"]), ctx


def test_render_rejects_and_empty(torch_cuda):
    """Mode 0 with r0 or n off the 64-row tile returns -1; n <= 0 returns 0; neither writes."""
    torch = torch_cuda
    A, KT = 7, 1
    X, mu, _ = OC.render_rows(130, A)
    src, dmu = _dev(torch, X.reshape(-1)), _dev(torch, mu)
    for (r0, n, mode), rc in (((32, 64, 0), -1), ((0, 100, 0), -1), ((0, 0, 0), 0),
                              ((0, -5, 1), 0), ((0, 64, 2), -1)):
        R = Render(torch, 192, 130, A, KT, min(mode, 1))
        R.mode = mode
        assert R.call(src, False, r0, n, 130, dmu) == rc, (r0, n, mode)
        R.guards("reject")
        for g in (R.img, R.xq, R.xrow, R.dst):
            g.untouched(np.ones(g.n, bool), f"render ({r0}, {n}, {mode})")
        assert list(R.w.get()) == [0, 0, 0, 0]
    R = Render(torch, 192, 130, A, 3, 0)             # no kernel for KT 3
    assert R.call(src, False, 0, 64, 130, dmu) == -1
    R.img.untouched(np.ones(R.img.n, bool), "render KT 3")


# ------------------------------------------------------------------ dmlp_rows_from_i32
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4099, len(OC.I32_EDGES) + (1 << 18)])
def test_rows_from_i32(torch_cuda, n):
    """dst[i] is the correctly rounded m / 1e6 (NumPy's division, pinned by the model test) for
    the vector body and the scalar tail; nothing behind dst[n) is written; a misaligned src or dst
    is rejected with nothing written."""
    torch = torch_cuda
    L = _lib.lib()
    m = OC.i32_values(n, seed=n)
    m[-1] = OC.I32_EDGES[n % len(OC.I32_EDGES)]          # an edge value in the tail too
    src = _dev(torch, np.concatenate([m, np.zeros(4, np.int32)]))
    dst = RC.guarded(torch, n, torch.float64)
    assert src.data_ptr() % 16 == 0 and dst.ptr() % 16 == 0
    assert L.dmlp_rows_from_i32(src.data_ptr() + 4, n, dst.ptr(), _stream(torch)) == -1
    assert L.dmlp_rows_from_i32(src.data_ptr(), n, dst.ptr() + 8, _stream(torch)) == -1
    dst.check_guards("misaligned")
    dst.untouched(np.ones(n, bool), "rows_from_i32 misaligned")
    assert L.dmlp_rows_from_i32(src.data_ptr(), n, dst.ptr(), _stream(torch)) == 0
    dst.check_guards(f"rows_from_i32 n={n}")
    np.testing.assert_array_equal(dst.host().view(np.uint64), OC.i32_rows(m).view(np.uint64))


def test_rows_i32_round_trip(torch_cuda):
    """six-decimal doubles -> dmlp_cpu_rows_i32 -> dmlp_rows_from_i32 are the input bits (the
    host accepts |m| <= 2^31 - 1)"""
    torch = torch_cuda
    L = _lib.lib()
    rng = np.random.default_rng(4)
    x = np.concatenate([np.round(rng.uniform(-2147.0, 2147.0, 4099), 6),
                        np.round(rng.uniform(0.0, 1000.0, 4096), 6),
                        [0.0, 1e-6, -1e-6, 999.999999, 2147.483647, -2147.483647, 5e-6]])
    x = np.ascontiguousarray(x)
    m = np.empty(len(x), np.int32)
    assert L.dmlp_cpu_rows_i32(x.ctypes.data, len(x), m.ctypes.data) == 0
    src = _dev(torch, m)
    dst = RC.guarded(torch, len(x), torch.float64)
    assert L.dmlp_rows_from_i32(src.data_ptr(), len(x), dst.ptr(), _stream(torch)) == 0
    dst.check_guards("round trip")
    np.testing.assert_array_equal(dst.host().view(np.uint64), x.view(np.uint64))


# ------------------------------------------------------------------ dmlp_x1_rowmajor
@pytest.mark.parametrize("n_tiles", [1, 3])
@pytest.mark.parametrize("KT", [1, 2, 4, 8])
def test_x1_rowmajor(torch_cuda, KT, n_tiles):
    """A distinct counter in every 16-byte chunk of the image: the output is rowmajor() of it."""
    torch = torch_cuda
    L = _lib.lib()
    nch = n_tiles * 64 * 4 * KT
    img = (np.arange(nch * 4, dtype=np.int32) + 1000).reshape(nch, 4)
    d = _dev(torch, img)
    out = RC.guarded(torch, (nch, 4), torch.int32)
    assert L.dmlp_x1_rowmajor(d.data_ptr(), n_tiles, KT, out.ptr(), _stream(torch)) == 0
    out.check_guards(f"rowmajor KT={KT}")
    np.testing.assert_array_equal(out.host(), OC.rowmajor(img, KT))


def test_x1_rowmajor_rejects(torch_cuda):
    torch = torch_cuda
    L = _lib.lib()
    d = _dev(torch, np.zeros((64 * 4 * 9, 4), np.int32))
    out = RC.guarded(torch, (64 * 4 * 9, 4), torch.int32)
    for n_tiles, KT, rc in ((1, 0, -1), (1, 9, -1), (0, 1, 0), (-1, 2, 0)):
        assert L.dmlp_x1_rowmajor(d.data_ptr(), n_tiles, KT, out.ptr(), _stream(torch)) == rc
    out.check_guards("rowmajor rejects")
    out.untouched(np.ones((64 * 4 * 9, 4), bool), "rowmajor rejects")


# ------------------------------------------------------------------ dmlp_center
@pytest.mark.parametrize("A", [1, 7, 33])
@pytest.mark.parametrize("N", [0, 1, 255, 257, 4096, 4097])
def test_center(torch_cuda, N, A):
    """mu = the mean of the first min(N, 4096) rows: row 4096 holds 1e12 and must not show."""
    torch = torch_cuda
    rng = np.random.default_rng(N * 7 + A)
    X = np.round(rng.uniform(-1000.0, 1000.0, (max(N, 1), A)), 6)
    if N > 4096:
        X[4096] = 1e12
    mu = RC.guarded(torch, A, torch.float64)
    dX = _dev(torch, X)
    assert _lib.lib().dmlp_center(dX.data_ptr(), N, A, mu.ptr(), _stream(torch)) == 0
    mu.check_guards(f"center N={N} A={A}")
    got = mu.host()
    n = min(N, 4096)
    if n == 0:
        assert (got == 0.0).all() and not np.signbit(got).any()
        return
    for a in range(A):
        col = X[:n, a].tolist()
        mean = sum(map(Fraction, col)) / n
        bound = Fraction((n + 1) * 2.0 ** -53) * Fraction(math.fsum(map(abs, col))) / n
        assert abs(Fraction(float(got[a])) - mean) <= bound, f"center N={N} A={A} column {a}"
