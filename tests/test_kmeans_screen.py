"""The screened k-means assignment (csrc/kmeans_screen.hip) on the GPU: kmeans_assign_gpu(...,
screen=True) and the estimators with assign="screen" against the NumPy reference of
tests/helpers/kmeans_contract.py and the CPU twin, bit for bit."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.models import KMeans, NearestCentroid
from distributed_machine_learning_project_amd.ops import knn as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import kmeans_contract as KC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def check_screened(torch, X, C, prev, ref):
    """two screened calls in a row against ref = (label, dmin, changed) and the CPU twin;
    returns the second call's stats"""
    Xd, Cd, pd = dev(torch, X), dev(torch, C), dev(torch, prev)
    runs = [K.kmeans_assign_gpu(Xd, Cd, pd, screen=True, stats=True) for _ in range(2)]
    torch.cuda.synchronize()
    for got in runs:
        for want in (ref, K.kmeans_assign_cpu(X, C, prev)):
            np.testing.assert_array_equal(got[0].cpu().numpy(), want[0])
            np.testing.assert_array_equal(KC.bits(got[1].cpu().numpy()), KC.bits(want[1]))
            assert int(got[2]) == want[2]
    return runs[1][3].cpu().numpy()


def tile_plus_one(A):
    return (65, A, _lib.lib().dmlp_kmeans_screen_tile(A) + 1)


# KT = 3 padded, KT = 4 (there 129 is one centroid more than an LDS tile holds), and one more
# than a tile at A = 32 and A = 64
EDGES = KC.ASSIGN + [(130, 65, 17), (65, 128, 129), "tile32", "tile64"]


@pytest.mark.parametrize("case", EDGES, ids=lambda c: c if isinstance(c, str) else
                         "-".join(map(str, c)))
def test_edges_and_escalation(torch_cuda, case):
    """ties at d = 0, an +inf centroid (every row escalates), an +inf row, N = 1"""
    if isinstance(case, str):
        case = tile_plus_one(int(case[4:]))
    X, C, prev, label, dmin, ndiff = KC.assign_case(*case)
    check_screened(torch_cuda, X, C, prev, (label, dmin, ndiff))


@pytest.mark.parametrize("A,Kc", [(17, 129), (32, 129), (33, 129), (65, 129), (128, 129),
                                  (32, 300)])
def test_screen_decides(torch_cuda, A, Kc):
    """well separated integer centroids: one candidate per row, nothing escalated"""
    rng = np.random.default_rng(0)
    N = 130
    C = rng.integers(-4, 5, (Kc, A)).astype(np.float64)
    own = rng.integers(0, Kc, N)
    X = C[own] + np.round(rng.uniform(-0.01, 0.01, (N, A)), 3)
    label, dmin = KC.ref_assign(X, C)
    prev = label.copy()
    prev[::3] += 1
    stats = check_screened(torch_cuda, X, C, prev, (label, dmin, len(prev[::3])))
    assert tuple(stats) == (0, N)


def test_overflow(torch_cuda):
    """129 identical centroids: every row's list overflows, the exact kernel answers"""
    rng = np.random.default_rng(1)
    X, C = np.round(rng.uniform(-4, 4, (65, 32)), 3), np.tile(rng.uniform(-4, 4, (1, 32)), (129, 1))
    label, dmin = KC.ref_assign(X, C)
    stats = check_screened(torch_cuda, X, C, label + 1, (label, dmin, 65))
    assert stats[0] == 65 and not label.any()


@pytest.mark.parametrize("fit", KC.FITS, ids=lambda f: f[0])
def test_kmeans_fit_screened(torch_cuda, fit):
    X, init, tol, _, _ = KC.fit_case(fit[0])
    km = KMeans(fit[2], init, tol=tol, device="gpu", assign="screen").fit(X)
    KC.check_fit(km, fit[0])
    cpu = KMeans(fit[2], init, tol=tol, device="cpu").fit(X)
    np.testing.assert_array_equal(KC.bits(km.cluster_centers_), KC.bits(cpu.cluster_centers_))
    assert (km.n_iter_, KC.bits(km.inertia_)) == (cpu.n_iter_, KC.bits(cpu.inertia_))


def test_nearest_centroid_and_row_reuse(torch_cuda):
    torch = torch_cuda
    X, label, _, _ = KC.sums_case(33)                       # (values of 1e16: rows that escalate)
    y = np.array([-7, 2, 40, 41, 90, 1000])[label]
    got = NearestCentroid(device="gpu", assign="screen").fit(X, y).predict(X[:50])
    np.testing.assert_array_equal(got, NearestCentroid(device="cpu").fit(X, y).predict(X[:50]))
    with pytest.raises(ValueError):
        NearestCentroid(assign="mfma")
    # one set of row operands against two different centroid sets
    X, C, _, label, dmin, _ = KC.assign_case(130, 33, 17)
    rows = K.kmeans_rows_gpu(dev(torch, X))
    for Cn in (C, C[::-1].copy()):
        lab, dm, ch = K.kmeans_assign_gpu(rows, dev(torch, Cn), screen=True)
        ref = KC.ref_assign(X, Cn)
        np.testing.assert_array_equal(lab.cpu().numpy(), ref[0])
        np.testing.assert_array_equal(KC.bits(dm.cpu().numpy()), KC.bits(ref[1]))
        assert ch is None


def test_empty_and_arguments(torch_cuda):
    """N = 0 and K = 0 launch nothing; A = 129 and null pointers: -1, the outputs untouched"""
    torch = torch_cuda
    L = _lib.lib()
    X, C, _, _, _, _ = KC.assign_case(65, 17, 16)
    Xd, Cd = dev(torch, X), dev(torch, C)
    lab, dmin, _ = K.kmeans_assign_gpu(Xd[:0], Cd, screen=True)
    assert lab.shape == (0,) and dmin.shape == (0,)
    assert L.dmlp_kmeans_screen_rows_bytes(65, 129) == -1
    assert L.dmlp_kmeans_screen_bytes(65, 129, 16) == -1
    rows = K.kmeans_rows_gpu(Xd).buf
    ws = torch.empty(L.dmlp_kmeans_screen_bytes(65, 17, 16), dtype=torch.uint8, device="cuda")
    out = torch.full((65,), -5, dtype=torch.int32, device="cuda")
    d = torch.zeros(65, dtype=torch.float64, device="cuda")
    st = torch.full((2,), -5, dtype=torch.int32, device="cuda")
    p = [rows.data_ptr(), rows.numel(), Xd.data_ptr(), 65, 17, Cd.data_ptr(), 16, None,
         out.data_ptr(), d.data_ptr(), None, st.data_ptr(), ws.data_ptr(), ws.numel(),
         torch.cuda.current_stream().cuda_stream]
    for i, bad in ((0, None), (1, 8), (2, None), (4, 129), (5, None), (8, None), (9, None),
                   (10, st.data_ptr()), (11, None), (12, None), (13, 8)):
        assert L.dmlp_kmeans_assign_screened(*(p[:i] + [bad] + p[i + 1:])) == -1, i
    assert L.dmlp_kmeans_assign_screened(*(p[:6] + [0] + p[7:])) == 0
    assert L.dmlp_kmeans_assign_screened(*(p[:3] + [0] + p[4:])) == 0
    torch.cuda.synchronize()
    assert (out == -5).all() and (st == -5).all()
    # A = 129 through the front end: the exact kernel's answer
    X, C, prev, label, dmin, ndiff = KC.assign_case(65, 129, 17)
    got = K.kmeans_assign_gpu(dev(torch, X), dev(torch, C), dev(torch, prev), screen=True,
                              stats=True)
    np.testing.assert_array_equal(got[0].cpu().numpy(), label)
    assert int(got[2]) == ndiff and not got[3].any()
