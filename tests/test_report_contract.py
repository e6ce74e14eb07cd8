"""Kernel-level contract of the report formatter (report.hip k_fmt_len / k_fmt_scan_blocks /
k_fmt_write) and of the two small fill kernels (merge.hip), through the C ABI.

The text goes into exactly dmlp_format_bound(nq) bytes and the scratch into exactly
dmlp_format_scratch(nq) int64, both between sentinel bands (tests/helpers/result_contract.py:
guarded); the text and line_off[0..nq] are compared with the Python-integer reference of
tests/helpers/operand_contract.py (pinned against dmlp_cpu_format_report by
tests/test_operand_contract_model.py) and every byte past line_off[nq] must keep its sentinel.
A report in chained parts (dmlp_format_report_at) must join to the whole report with part
boundaries at byte offsets 1, 2 and 3 modulo 4, in either order of issue.  All comparisons are
bit-exact."""
import os
import sys

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


def _cs_dev(torch, cs):
    return _dev(torch, np.ascontiguousarray(cs).view(np.int64))


class Report:
    """Guarded text of `bound` bytes (default: exactly dmlp_format_bound(nq))."""

    def __init__(self, torch, nq, bound=None):
        L = _lib.lib()
        self.torch = torch
        self.bound = int(L.dmlp_format_bound(nq)) if bound is None else bound
        self.out = RC.guarded(torch, self.bound, torch.uint8)

    def scratch(self, nq):
        n = int(_lib.lib().dmlp_format_scratch(nq))
        assert n >= nq + 1
        return RC.guarded(self.torch, n, self.torch.int64)

    def check(self, text: bytes, start, ctx):
        """bytes [start, start + len(text)) == text, every other byte holds its sentinel"""
        self.out.check_guards(ctx + " text")
        h = self.out.host()
        got = bytes(h[start:start + len(text)])
        if got != text:
            i = next(j for j in range(len(text)) if got[j] != text[j])
            raise AssertionError(f"{ctx}: text differs at byte {start + i}: "
                                 f"{got[max(0, i - 30):i + 30]!r} != {text[max(0, i - 30):i + 30]!r}")
        keep = np.ones(self.bound, bool)
        keep[start:start + len(text)] = False
        self.out.untouched(keep, ctx + " bytes outside the text")


def run_report(torch, cs, qid_base, ctx):
    L = _lib.lib()
    nq = len(cs)
    rep = Report(torch, nq)
    off = rep.scratch(nq)
    d = _cs_dev(torch, cs)
    assert L.dmlp_format_report(d.data_ptr(), nq, qid_base, off.ptr(), rep.out.ptr(),
                                _stream(torch)) == 0, ctx
    off.check_guards(ctx + " scratch")
    text = OC.report_ref(cs, qid_base)
    np.testing.assert_array_equal(off.host()[:nq + 1], OC.line_offsets_ref(cs, qid_base),
                                  err_msg=ctx + " line_off")
    rep.check(text, 0, ctx)


QID_BASES = (0, 9, 99, 999_999, 10 ** 9 - 3)


@pytest.mark.parametrize("nq", [1, 2, 255, 256, 257, 1000])
def test_format_report_contract(torch_cuda, nq):
    """Every digit count of the checksum (its ends, zero nine-digit groups), every digit boundary
    of the query id inside a run, block boundaries of the 256-line blocks."""
    for base in (*QID_BASES, 2 ** 31 - 1 - nq):
        cs = OC.checksums(nq, seed=base % 1000)
        if nq <= 2:      # the extremes where one line is the whole report
            for pair in ((0, 2 ** 64 - 1), (10 ** 9, 10 ** 18), (10 ** 19, 9)):
                run_report(torch_cuda, np.array(pair[:nq], np.uint64), base,
                           f"format nq={nq} base={base} cs={pair[:nq]}")
        run_report(torch_cuda, cs, base, f"format nq={nq} base={base}")


def test_format_report_second_scan_pass(torch_cuda):
    """1024 * 256 + 257 lines: more than 1024 blocks, the carry of k_fmt_scan_blocks."""
    nq = 1024 * 256 + 257
    run_report(torch_cuda, OC.checksums(nq, seed=1), 999_999, f"format nq={nq}")


def split_points(off, residues, mins):
    """indices n1 < n2 < n3 with off[n_i] % 4 == residues[i] and n_i >= n_(i-1) + mins[i]"""
    out, prev = [], 0
    for r, mn in zip(residues, mins):
        n = next(i for i in range(prev + mn, len(off)) if off[i] % 4 == r)
        out.append(n)
        prev = n
    return out


@pytest.mark.parametrize("residues", [(1, 2, 3), (3, 1, 2), (2, 3, 1)])
@pytest.mark.parametrize("qid_base", [0, 99_990])
def test_format_report_at_parts(torch_cuda, residues, qid_base):
    """Three parts of uneven size (257+, 100+, 300+ lines) whose ends fall at byte offsets
    `residues` modulo 4.  Chained on the device (each base the previous part's line_off[nq]) and,
    with the bases precomputed, issued last to first: the joined text is the whole report, every
    line_off is absolute and no part touches a byte of its neighbours or past the text."""
    torch = torch_cuda
    L = _lib.lib()
    pool = OC.checksums(1200, seed=sum(residues) + qid_base)
    n1, n2, n3 = split_points(OC.line_offsets_ref(pool, qid_base), residues, (257, 100, 300))
    cs = pool[:n3]
    ref_off = OC.line_offsets_ref(cs, qid_base)
    assert [int(ref_off[n]) % 4 for n in (n1, n2, n3)] == list(residues)
    text = OC.report_ref(cs, qid_base)
    parts = [(0, n1), (n1, n2), (n2, n3)]
    d = _cs_dev(torch, cs)
    for order in ("chained", "reversed"):
        ctx = f"format_at {residues} base={qid_base} {order}"
        rep = Report(torch, n3)
        scr = [rep.scratch(b - a) for a, b in parts]
        if order == "chained":
            bases = [None] + [scr[i].ptr() + 8 * (parts[i][1] - parts[i][0]) for i in range(2)]
            seq = (0, 1, 2)
        else:
            pre = _dev(torch, np.array([ref_off[a] for a, _ in parts], np.int64))
            bases = [pre.data_ptr() + 8 * i for i in range(3)]
            seq = (2, 1, 0)
        for i in seq:
            a, b = parts[i]
            assert L.dmlp_format_report_at(d.data_ptr() + 8 * a, b - a, qid_base + a, scr[i].ptr(),
                                           rep.out.ptr(), bases[i], _stream(torch)) == 0, ctx
        for i, (a, b) in enumerate(parts):
            scr[i].check_guards(f"{ctx} scratch {i}")
            np.testing.assert_array_equal(scr[i].host()[:b - a + 1], ref_off[a:b + 1],
                                          err_msg=f"{ctx}: line_off of part {i}")
        rep.check(text, 0, ctx)


def test_format_report_at_base_only(torch_cuda):
    """One part at bases 1, 2, 3 and 5: the bytes before the base keep their sentinel too."""
    torch = torch_cuda
    L = _lib.lib()
    cs = OC.checksums(300, seed=8)
    text = OC.report_ref(cs, 7)
    d = _cs_dev(torch, cs)
    for b in (1, 2, 3, 5):
        rep = Report(torch, 300)
        off = rep.scratch(300)
        base = _dev(torch, np.array([b], np.int64))
        assert L.dmlp_format_report_at(d.data_ptr(), 300, 7, off.ptr(), rep.out.ptr(),
                                       base.data_ptr(), _stream(torch)) == 0
        off.check_guards(f"format_at base {b}")
        np.testing.assert_array_equal(off.host()[:301], OC.line_offsets_ref(cs, 7, b))
        rep.check(text, b, f"format_at base {b}")


def test_format_report_empty_and_misaligned(torch_cuda):
    """nq <= 0 returns 0; an out that is not 4-byte aligned returns -1 before any launch (the
    dword stores of k_fmt_write are aligned on the byte offset, not on the address); neither
    writes the text or the scratch."""
    torch = torch_cuda
    L = _lib.lib()
    cs = OC.checksums(300, seed=2)
    d = _cs_dev(torch, cs)
    rep = Report(torch, 300)
    off = rep.scratch(300)
    assert rep.out.ptr() % 4 == 0
    for nq in (0, -3):
        assert L.dmlp_format_report(d.data_ptr(), nq, 0, off.ptr(), rep.out.ptr(),
                                    _stream(torch)) == 0
        assert L.dmlp_format_report_at(d.data_ptr(), nq, 0, off.ptr(), rep.out.ptr(), None,
                                       _stream(torch)) == 0
    for k in (1, 2, 3):
        assert L.dmlp_format_report(d.data_ptr(), 300, 0, off.ptr(), rep.out.ptr() + k,
                                    _stream(torch)) == -1
        assert L.dmlp_format_report_at(d.data_ptr(), 300, 0, off.ptr(), rep.out.ptr() + k, None,
                                       _stream(torch)) == -1
    rep.check(b"", 0, "format rejects")
    off.check_guards("format rejects scratch")
    off.untouched(np.ones(off.n, bool), "format rejects scratch")


# ------------------------------------------------------------------ dmlp_fill_f64 / _offset_ids
FILL_N = [0, 1, 255, 257, 4096 * 256 + 1]      # the last: the grid stride wraps (4096 blocks)


@pytest.mark.parametrize("n", FILL_N)
def test_fill_f64(torch_cuda, n):
    torch = torch_cuda
    L = _lib.lib()
    for v in (np.inf, -2.5):
        buf = RC.guarded(torch, n + 3, torch.float64)
        assert L.dmlp_fill_f64(buf.ptr(), n, v, _stream(torch)) == 0
        buf.check_guards(f"fill n={n}")
        assert (buf.host()[:n] == v).all(), f"fill n={n} v={v}"
        buf.untouched(np.arange(n + 3) >= n, f"fill n={n}")
    buf = RC.guarded(torch, 4, torch.float64)
    assert L.dmlp_fill_f64(buf.ptr(), -1, 1.0, _stream(torch)) == 0
    buf.untouched(np.ones(4, bool), "fill n=-1")


@pytest.mark.parametrize("n", FILL_N)
def test_offset_ids(torch_cuda, n):
    """every id >= 0 (0 included) is shifted, every -1 kept; off = 0 changes nothing"""
    torch = torch_cuda
    L = _lib.lib()
    rng = np.random.default_rng(n)
    ids = rng.integers(-1, 1000, n + 3).astype(np.int32)
    ids[rng.integers(0, n + 3, (n + 3) // 4)] = -1
    ids[::5] = 0
    if n:
        ids[n - 1] = 0
    for off in (7, 0, 1 << 20):
        buf = RC.guarded(torch, n + 3, torch.int32)
        buf.t.copy_(torch.from_numpy(ids))
        assert L.dmlp_offset_ids(buf.ptr(), n, off, _stream(torch)) == 0
        buf.check_guards(f"offset_ids n={n}")
        want = ids.copy()
        want[:n] = np.where(ids[:n] >= 0, ids[:n] + off, ids[:n])
        np.testing.assert_array_equal(buf.host(), want, err_msg=f"offset_ids n={n} off={off}")
