"""Pins the references of tests/helpers/operand_contract.py (CPU only), so that a failure of
tests/test_operand_contract.py or tests/test_report_contract.py is the kernel's: the bf16
rounding against torch's cast, the render model against host_prep.cpp bit for bit, the report
against dmlp_cpu_format_report, the point-major copy, and NumPy's int32 / 1e6 against the exact
quotient.  Each also shows that the value it pins discriminates (the wrong variant differs)."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import operand_contract as OC  # noqa: E402


def test_bf16_rne_matches_torch():
    import torch
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 32, 1 << 16, dtype=np.int64).astype(np.uint32)
    k = np.arange(1 << 10, dtype=np.uint32)
    edge = np.concatenate([
        (0x3f80 + k << np.uint32(16)) | np.uint32(0x8000),           # ties, even and odd LSB
        (0x3f80 + k << np.uint32(16)) | np.uint32(0x7fff),
        (0x3f80 + k << np.uint32(16)) | np.uint32(0x8001),
        np.array([0x3fffffff, 0x40000000, 0x3fff8000, 0x3fff7fff,    # both sides of a binade edge
                  0x007fffff, 0x00800000, 0x007f8000, 0x00008000, 0x00008001, 0x00000001,
                  0x00018000, 0x00000000, 0x80000000, 0x7f7fffff, 0x7f800000], np.uint32)])
    edge = np.concatenate([edge, edge | np.uint32(0x80000000)])
    u = np.concatenate([bits, edge]).astype(np.uint32)
    f = u.view(np.float32)
    f = f[~np.isnan(f)]
    want = torch.from_numpy(f.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(OC.bf16_rne(f), want)
    assert (OC.bf16_trunc(f) != want).any()


def test_split_bf16_properties():
    """hi + lo reproduces c to 2^-16 relative (or the bf16 subnormal step), and the edge set holds
    what its comments say: ties both ways, a lo decided below fp32(c), a hi in the next binade."""
    e = OC.bf16_edges()
    hi, lo = OC.split_bf16(e)
    err = np.abs(OC.bf16_to_f64(hi) + OC.bf16_to_f64(lo) - e)
    assert (err <= np.maximum(np.abs(e) * 2.0 ** -16, 2.0 ** -134)).all()
    assert (OC.bf16_trunc(e.astype(np.float32)) != hi).any()
    # lo from fp32(c) - hi instead of the fp64 difference differs on this set
    f = e.astype(np.float32)
    lo32 = OC.bf16_rne(f - OC.bf16_to_f64(hi).astype(np.float32))
    assert (lo32 != lo).any()
    h2, _ = OC.split_bf16(np.array([2.0 - 2.0 ** -9]))
    assert h2[0] == 0x4000
    assert OC.split_bf16(np.array([-0.0]))[0][0] == 0x8000


def _cpu_queries(L, Qx, mu, KT):
    Q, A = Qx.shape
    hh = np.full((Q, KT * 32), 7, np.uint16)
    qn = np.full(Q, -1.0, np.float32)
    rc = L.dmlp_cpu_prep_queries(Qx.ctypes.data, Q, A, mu.ctypes.data, KT, hh.ctypes.data,
                                 qn.ctypes.data)
    return rc, hh, qn


@pytest.mark.parametrize("A", [7, 32, 40, 100, 200, 256])
@pytest.mark.parametrize("i32", [False, True])
def test_render_model_matches_host(A, i32):
    """render_model == dmlp_cpu_prep_data / dmlp_cpu_prep_queries bit for bit on the adversarial
    sets: the AVX2 shapes (A % 8 == 0) and the scalar ones."""
    L = _lib.lib()
    KT = 1 if A <= 32 else 2 if A <= 64 else 4 if A <= 128 else 8
    n = 130
    X, mu, _ = OC.render_rows(n, A, i32=i32)
    rc, hh, qn = _cpu_queries(L, X, mu, KT)
    m1 = OC.render_model(X, mu, KT, 1)
    assert rc == 0 and m1["bad"] == 0
    np.testing.assert_array_equal(hh, m1["img"])
    np.testing.assert_array_equal(qn.view(np.uint32), m1["xq"].view(np.uint32))
    if not i32:   # one accumulator instead of four: fp32 sees it on order_row's rows only
        assert (OC.render_model(X, mu, KT, 1, single=True)["xq"] != qn).any()
    nt = (n + 63) // 64
    img = np.full(nt * 64 * KT * 32, 7, np.uint16)
    xin = np.zeros(nt * 64, np.float32)
    nm = np.zeros(1, np.uint32)
    assert L.dmlp_cpu_prep_data(X.ctypes.data, n, A, mu.ctypes.data, KT, img.ctypes.data,
                                xin.ctypes.data, nm.ctypes.data) == 0
    m0 = OC.render_model(X, mu, KT, 0)
    np.testing.assert_array_equal(img, m0["img"])
    np.testing.assert_array_equal(xin.view(np.uint32), m0["xq"].view(np.uint32))
    assert int(nm[0]) == OC.nmax_bits(m0["up"])


@pytest.mark.parametrize("A", [7, 32])
def test_render_model_flags(A):
    L = _lib.lib()
    X, mu, _ = OC.render_rows(20, A)
    for v in OC.FP16_FLAGS:
        for r, a in ((0, 0), (19, 0), (7, A - 1)):
            Y = X.copy()
            Y[r, a] = v + mu[a]                      # (65504.5 is exact: c = 65504)
            rc, hh, qn = _cpu_queries(L, Y, mu, 1)
            m = OC.render_model(Y, mu, 1, 1)
            assert rc == 1 and m["bad"] == 1
            assert m["img"][r, a] == 0
            np.testing.assert_array_equal(hh, m["img"])
            np.testing.assert_array_equal(qn.view(np.uint32), m["xq"].view(np.uint32))


def test_report_ref_matches_host():
    L = _lib.lib()
    for nq, base in ((1, 0), (257, 9), (1000, 999_999), (300, 10 ** 9 - 3),
                     (500, 2 ** 31 - 1 - 500)):
        cs = OC.checksums(nq, seed=nq)
        out = np.zeros(48 * nq, np.uint8)
        n = L.dmlp_cpu_format_report(cs.ctypes.data, nq, base, out.ctypes.data)
        ref = OC.report_ref(cs, base)
        assert bytes(out[:n]) == ref
        off = OC.line_offsets_ref(cs, base, 5)
        assert off[0] == 5 and off[-1] == 5 + len(ref) and len(off) == nq + 1
    lens = {len(str(int(c))) for c in OC.checksum_values()}
    assert lens == set(range(1, 21))


@pytest.mark.parametrize("KT", [1, 2, 4, 8])
def test_rowmajor_is_attribute_order(KT):
    n, W = 192, KT * 32
    rows = (np.arange(n * W) % 65521).astype(np.uint16).reshape(n, W)
    img = OC.hi_image(rows, KT)
    back = OC.rowmajor(img.reshape(-1, 8), KT).reshape(n, W)
    np.testing.assert_array_equal(back, rows)


def test_i32_quotient_is_correctly_rounded():
    """x = m / 1e6 in NumPy is the double nearest to the exact quotient (no neighbour is as near:
    10^6 q is an integer, so a tie cannot occur but at q = 0) over the int32 set of the GPU test;
    m * 1e-6 is not."""
    m = OC.i32_values(len(OC.I32_EDGES) + (1 << 18), seed=3)
    x = OC.i32_rows(m)
    assert (m.astype(np.float64) * 1.0e-6 != x).any()
    lo, hi = np.nextafter(x, -np.inf), np.nextafter(x, np.inf)
    M = 10 ** 6
    for mi, xi, li, hj in zip(m.tolist(), x.tolist(), lo.tolist(), hi.tolist()):
        n, d = xi.as_integer_ratio()
        e = abs(n * M - mi * d)                      # |x - q| = e / (d M)
        for y in (li, hj):
            ny, dy = y.as_integer_ratio()
            assert e * dy < abs(ny * M - mi * dy) * d, (mi, xi)
    # the same claim through fractions.Fraction on the edge values
    for mi in OC.I32_EDGES.tolist():
        xi = float(OC.i32_rows(np.array([mi]))[0])
        q = Fraction(mi, M)
        for y in (np.nextafter(xi, -np.inf), np.nextafter(xi, np.inf)):
            assert abs(Fraction(xi) - q) < abs(Fraction(float(y)) - q)
