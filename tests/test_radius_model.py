"""The radius search on the host: tests/helpers/radius_contract.py's reference pinned bit for bit
against the CPU twins (dmlp_cpu_radius_count, dmlp_cpu_radius_fill in both orders), against
ops.reference.radius_reference and against the k-NN reference at k = count (a query's neighbours
are the head of its k-NN list); the near-tie inputs, whose membership depends on the summation
order; the CSR and padded layouts with untouched padding; the argument errors; the wrappers'
ValueErrors."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.ops import knn as K
from distributed_machine_learning_project_amd.ops import reference as REF

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import radius_contract as RR  # noqa: E402
import result_contract as RC  # noqa: E402

FILL_D, FILL_I, BAND = -7.0, -12345, 64


def _case(kind, args):
    case = {"grid": RR.grid_case, "equal": RR.all_equal_case, "tie": RR.near_tie_case}[kind](*args)
    return case[:3], RR.ref_of(kind, *args)


def _cpu_count(X, Qx, r2, N=None, A=None, nq=None, nulls=(), out=None):
    out = np.full(len(Qx) + 2 * BAND, FILL_I, np.int32) if out is None else out
    p = {"X": X.ctypes.data, "Qx": Qx.ctypes.data, "r2": r2.ctypes.data,
         "out": out[BAND:].ctypes.data}
    for n in nulls:
        p[n] = None
    rc = _lib.lib().dmlp_cpu_radius_count(
        p["X"], X.shape[0] if N is None else N, X.shape[1] if A is None else A, p["Qx"],
        len(Qx) if nq is None else nq, p["r2"], p["out"], 2)
    return rc, out


def _cpu_fill(X, Qx, r2, count, off, size, sort, fill=(FILL_D, FILL_I), N=None, A=None, nq=None,
              nulls=()):
    d = np.full(size + 2 * BAND, fill[0], np.float64)
    i = np.full(size + 2 * BAND, fill[1], np.int32)
    count = np.ascontiguousarray(count, np.int32)
    off = np.ascontiguousarray(off, np.int64)
    p = {"X": X.ctypes.data, "Qx": Qx.ctypes.data, "r2": r2.ctypes.data,
         "count": count.ctypes.data, "off": off.ctypes.data, "d": d[BAND:].ctypes.data,
         "i": i[BAND:].ctypes.data}
    for n in nulls:
        p[n] = None
    rc = _lib.lib().dmlp_cpu_radius_fill(
        p["X"], X.shape[0] if N is None else N, X.shape[1] if A is None else A, p["Qx"],
        len(Qx) if nq is None else nq, p["r2"], p["count"], p["off"], p["d"], p["i"], sort, 2)
    return rc, d, i


def _check_flat(d, i, segs, off, size, ctx, fill=(FILL_D, FILL_I), count=None):
    """the payload holds the segments and its fill everywhere else; the bands their fill"""
    ed, ei = RR.expected(segs, off, size, fill[0], fill[1], count)
    assert RR.same_bits(d[BAND:BAND + size], ed), f"{ctx}: dist"
    assert RR.same_bits(i[BAND:BAND + size], ei), f"{ctx}: ids"
    for a, f in ((d, fill[0]), (i, fill[1])):
        assert (a[:BAND] == f).all() and (a[BAND + size:] == f).all(), f"{ctx}: band written"


CASES = [("grid", s) for s in RR.SHAPES] + [("grid", (1, 1, 7, r)) for r in (1, 3, 5)] + \
        [("equal", ())] + [("tie", (A,)) for A in RR.NEAR_TIE_AS]


@pytest.mark.parametrize("kind,args", CASES)
def test_cpu_twins_match_reference(kind, args):
    """counts as integers; CSR segments on their bits in both orders; untouched bands"""
    (X, Qx, r2), (count, srt, desc) = _case(kind, args)
    rc, out = _cpu_count(X, Qx, r2)
    assert rc == 0
    np.testing.assert_array_equal(out[BAND:BAND + len(Qx)], count)
    assert (out[:BAND] == FILL_I).all() and (out[BAND + len(Qx):] == FILL_I).all()
    off, total = RR.csr_offsets(count)
    for sort, segs in ((0, desc), (1, srt)):
        rc, d, i = _cpu_fill(X, Qx, r2, count, off, total, sort)
        assert rc == 0
        _check_flat(d, i, segs, off, total, f"{kind} {args} sort {sort}")


@pytest.mark.parametrize("kind,args", [("grid", (300, 65, 33)), ("grid", (129, 130, 7)),
                                       ("equal", ())])
def test_padded_layout(kind, args):
    """off = q * stride into lists pre-filled with (+inf, -1): the padding stays as it was"""
    (X, Qx, r2), (count, srt, desc) = _case(kind, args)
    stride = int(count.max()) + 3
    off = np.arange(len(Qx), dtype=np.int64) * stride
    for sort, segs in ((0, desc), (1, srt)):
        rc, d, i = _cpu_fill(X, Qx, r2, count, off, len(Qx) * stride, sort, fill=(np.inf, -1))
        assert rc == 0
        _check_flat(d, i, segs, off, len(Qx) * stride, f"{kind} sort {sort}", fill=(np.inf, -1))
        wd, wi, wc = K.radius_cpu(X, Qx, r2, sort=bool(sort), stride=stride)
        assert RR.same_bits(wd.ravel(), d[BAND:BAND + len(Qx) * stride])
        assert RR.same_bits(wi.ravel(), i[BAND:BAND + len(Qx) * stride])
        np.testing.assert_array_equal(wc, count)


def test_count_one_too_small():
    """a count below the hits drops the LARGEST ids (the last to arrive); nothing is written outside
    the shortened segments"""
    (X, Qx, r2), (count, srt, desc) = _case("grid", (300, 65, 33))
    small = np.maximum(count - 1, 0)
    off, total = RR.csr_offsets(small)
    kept = [(sd[1:], si[1:]) for sd, si in desc]
    rc, d, i = _cpu_fill(X, Qx, r2, small, off, total, 0)
    assert rc == 0
    _check_flat(d, i, kept, off, total, "one too small")


@pytest.mark.parametrize("kind,args", CASES)
def test_reference_implementations_agree(kind, args):
    """radius_contract.reference == ops.reference.radius_reference == the wrappers, in CSR"""
    (X, Qx, r2), (count, srt, desc) = _case(kind, args)
    off, total = RR.csr_offsets(count)
    for sort, segs in ((False, desc), (True, srt)):
        ed, ei = RR.expected(segs, off, total, 0.0, 0)
        indptr, d, i = REF.radius_reference(X, Qx, r2, sort=sort)
        np.testing.assert_array_equal(indptr[:-1], off)
        assert indptr[-1] == total and RR.same_bits(d, ed) and RR.same_bits(i, ei)
        indptr, d, i = K.radius_cpu(X, Qx, r2, sort=sort)
        np.testing.assert_array_equal(indptr[:-1], off)
        assert indptr[-1] == total and RR.same_bits(d, ed) and RR.same_bits(i, ei)
    np.testing.assert_array_equal(K.radius_count_cpu(X, Qx, r2), count)


@pytest.mark.parametrize("kind,args", CASES)
def test_prefix_identity(kind, args):
    """the sorted neighbours are the first count entries of the k-NN reference at k = count"""
    (X, Qx, r2), (count, srt, _) = _case(kind, args)
    ks = max(1, int(count.max()))
    kd, ki = RC.knn_ref(X, Qx, count, ks)
    for q, (sd, si) in enumerate(srt):
        assert RR.same_bits(kd[q, :count[q]], sd) and RR.same_bits(ki[q, :count[q]], si), q


def test_special_radii():
    """+inf keeps every real point, one at distance +inf included; NaN and negative keep nothing;
    0 keeps exact duplicates"""
    X, Qx, _ = RR.grid_case(300, 65, 33)
    d = np.array([RC.dist_l2r(q, X) for q in Qx])
    assert np.isinf(d).any()
    for v, want in ((np.inf, np.full(65, 300)), (np.nan, np.zeros(65)), (-1.0, np.zeros(65)),
                    (-np.inf, np.zeros(65)), (0.0, (d == 0).sum(axis=1)),
                    (1.7e308, np.isfinite(d).sum(axis=1))):
        np.testing.assert_array_equal(K.radius_count_cpu(X, Qx, v), want, err_msg=str(v))
    assert (d == 0).sum() > 30


@pytest.mark.parametrize("A", RR.NEAR_TIE_AS)
def test_near_ties_depend_on_the_summation_order(A):
    """r2[0] sits between distances that differ only by the rounding of the left-to-right sum: a
    right-to-left or a pairwise sum changes the membership, and so does one ulp of r2"""
    X, Qx, r2, b0 = RR.near_tie_case(A)
    d = RC.dist_l2r(Qx[0], X)
    block = d[b0:b0 + 160]
    assert 3 <= len(np.unique(block)) <= 10
    member = d <= r2[0]
    for wrong in (RC.dist_r2l, RC.dist_pairwise):
        assert ((wrong(Qx[0], X) <= r2[0]) != member).sum() >= 1, wrong.__name__
    c = int(member.sum())
    lo = int((d <= np.nextafter(r2[0], -np.inf)).sum())
    hi = int((d <= np.nextafter(r2[0], np.inf)).sum())
    assert lo < c <= hi and hi - lo >= 28
    assert K.radius_count_cpu(X, Qx, r2)[0] == c


def test_argument_errors_write_nothing():
    (X, Qx, r2), (count, _, desc) = _case("grid", (129, 65, 7))
    off, total = RR.csr_offsets(count)
    for kw in (dict(N=1 << 31), dict(A=0), dict(A=-1), dict(nulls=("X",)), dict(nulls=("Qx",)),
               dict(nulls=("r2",)), dict(nulls=("out",))):
        rc, out = _cpu_count(X, Qx, r2, **kw)
        assert rc == -1 and (out == FILL_I).all(), kw
    for kw in (dict(N=1 << 31), dict(A=0), dict(nulls=("X",)), dict(nulls=("Qx",)),
               dict(nulls=("r2",)), dict(nulls=("count",)), dict(nulls=("off",)),
               dict(nulls=("d",)), dict(nulls=("i",))):
        rc, d, i = _cpu_fill(X, Qx, r2, count, off, total, 1, **kw)
        assert rc == -1 and (d == FILL_D).all() and (i == FILL_I).all(), kw
    # nq <= 0 and N <= 0 return 0; the count entry still writes nq zeros for N <= 0
    for nq in (0, -3):
        rc, out = _cpu_count(X, Qx, r2, nq=nq)
        assert rc == 0 and (out == FILL_I).all()
        rc, d, i = _cpu_fill(X, Qx, r2, count, off, total, 1, nq=nq)
        assert rc == 0 and (d == FILL_D).all() and (i == FILL_I).all()
    for N in (0, -1):
        rc, out = _cpu_count(X, Qx, r2, N=N, nulls=("X",))
        assert rc == 0 and (out[BAND:BAND + len(Qx)] == 0).all()
        assert (out[:BAND] == FILL_I).all() and (out[BAND + len(Qx):] == FILL_I).all()
        rc, d, i = _cpu_fill(X, Qx, r2, count, off, total, 1, N=N)
        assert rc == 0 and (d == FILL_D).all() and (i == FILL_I).all()


def test_wrapper_value_errors():
    X, Qx, r2 = RR.grid_case(129, 65, 7)
    count = K.radius_count_cpu(X, Qx, r2)
    with pytest.raises(ValueError):
        K.radius_count_cpu(X, Qx[:, :5], r2)            # attribute counts differ
    with pytest.raises(ValueError):
        K.radius_count_cpu(X[0], Qx, r2)                # X not 2-d
    with pytest.raises(ValueError):
        K.radius_count_cpu(X, Qx, r2[:-1])              # r2 not [Q]
    with pytest.raises(ValueError):
        K.radius_cpu(X, Qx, r2, count=count[:-1])
    with pytest.raises(ValueError):
        K.radius_cpu(X, Qx, r2, stride=int(count.max()) - 1)   # a count above the stride
    with pytest.raises(ValueError):
        K.radius_cpu(X, Qx, r2, stride=0)
    with pytest.raises(ValueError):
        K._radius_layout(5, 1 << 31, 3, None)           # a span of 2^31
    with pytest.raises(ValueError):
        K._radius_layout(5, 0, 1 << 20, 1 << 12)
    # strided inputs and a scalar radius are taken
    Xs = np.asfortranarray(X)
    np.testing.assert_array_equal(K.radius_count_cpu(Xs, Qx[::2], 2.0),
                                  K.radius_count_cpu(X, np.ascontiguousarray(Qx[::2]),
                                                     np.full(len(Qx[::2]), 2.0)))
    # empty inputs
    indptr, d, i = K.radius_cpu(X, Qx[:0], r2[:0])
    assert indptr.tolist() == [0] and d.shape == (0,) and i.shape == (0,)
    assert K.radius_count_cpu(X[:0], Qx, np.inf).tolist() == [0] * len(Qx)
