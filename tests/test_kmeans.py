"""GPU tier of k-means (csrc/kmeans.hip): dmlp_kmeans_assign at both tile widths and
dmlp_cluster_sums through ops.knn, KMeans and NearestCentroid on the GPU path — against the NumPy
reference of tests/helpers/kmeans_contract.py and the CPU twins, bit for bit."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.models import KMeans
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


@pytest.mark.parametrize("pj", [1, 8])
@pytest.mark.parametrize("case", KC.ASSIGN, ids=lambda c: "-".join(map(str, c)))
def test_assign(torch_cuda, case, pj):
    """both tiles on every shape, whatever the dispatch by K picks"""
    torch = torch_cuda
    X, C, prev, label, dmin, ndiff = KC.assign_case(*case)
    Xd, Cd, pd = dev(torch, X), dev(torch, C), dev(torch, prev)
    old = _lib.lib().dmlp_set_kmeans_tile(pj)
    try:
        runs = [K.kmeans_assign_gpu(Xd, Cd, pd) for _ in range(2)]
        torch.cuda.synchronize()
    finally:
        _lib.lib().dmlp_set_kmeans_tile(old)
    cpu = K.kmeans_assign_cpu(X, C, prev)
    for got in runs:                                    # (the second call: the same bits)
        for ref in ((label, dmin, ndiff), cpu):
            np.testing.assert_array_equal(got[0].cpu().numpy(), ref[0])
            np.testing.assert_array_equal(got[1].cpu().numpy(), ref[1])
            assert int(got[2]) == ref[2]
    assert K.kmeans_assign_gpu(Xd, Cd)[2] is None


@pytest.mark.parametrize("A", [1, 33, 65])
@pytest.mark.parametrize("with_extra", [False, True])
def test_cluster_sums(torch_cuda, A, with_extra):
    torch = torch_cuda
    X, label, Kc, extra = KC.sums_case(A)
    extra = extra if with_extra else None
    ref = KC.ref_sums(X, label, Kc, extra)
    Cd = torch.full((Kc, A), 7.0, dtype=torch.float64, device="cuda")
    args = (dev(torch, X), dev(torch, label), Kc, None if extra is None else dev(torch, extra))
    sums, count = K.cluster_sums_gpu(*args, centroids=Cd)
    np.testing.assert_array_equal(KC.bits(sums.cpu().numpy()), KC.bits(ref))
    np.testing.assert_array_equal(KC.bits(sums.cpu().numpy()),
                                  KC.bits(K.cluster_sums_cpu(X, label, Kc, extra)[0]))
    np.testing.assert_array_equal(count.cpu().numpy(), [0, 1, 63, 64, 65, 129])
    C, n = Cd.cpu().numpy(), count.cpu().numpy()
    np.testing.assert_array_equal(KC.bits(C[1:]), KC.bits(ref[1:, :A] / n[1:, None]))
    assert (C[0] == 7.0).all()
    again = K.cluster_sums_gpu(*args)[0]                # (no Lloyd step; the same bits)
    np.testing.assert_array_equal(KC.bits(again.cpu().numpy()), KC.bits(ref))


@pytest.mark.parametrize("fit", KC.FITS, ids=lambda f: f[0])
def test_kmeans_fit(torch_cuda, fit):
    X, init, tol, _, _ = KC.fit_case(fit[0])
    km = KMeans(fit[2], init, tol=tol, device="gpu").fit(X)
    KC.check_fit(km, fit[0])
    cpu = KMeans(fit[2], init, tol=tol, device="cpu").fit(X)
    np.testing.assert_array_equal(KC.bits(km.cluster_centers_), KC.bits(cpu.cluster_centers_))
    assert (km.n_iter_, KC.bits(km.inertia_)) == (cpu.n_iter_, KC.bits(cpu.inertia_))


def test_nearest_centroid(torch_cuda):
    KC.check_nearest_centroid("gpu")


def test_empty_and_arguments(torch_cuda):
    """N = 0 and K = 0 launch nothing; -1 before any launch for what dmlp.h lists"""
    torch = torch_cuda
    L = _lib.lib()
    X, C, prev, label, _, _ = KC.assign_case(65, 17, 16)
    Xd, Cd = dev(torch, X), dev(torch, C)
    lab, dmin, _ = K.kmeans_assign_gpu(Xd[:0], Cd)
    assert lab.shape == (0,) and dmin.shape == (0,)
    sums, count = K.cluster_sums_gpu(Xd[:0], dev(torch, label[:0]), 4)
    assert not sums.any() and sums.shape == (4, 17) and not count.any()
    with pytest.raises(ValueError):
        K.kmeans_assign_gpu(Xd, Cd[:0])
    with pytest.raises(ValueError):
        K.kmeans_assign_gpu(Xd, Cd[:, :5])
    out = torch.full((65,), -5, dtype=torch.int32, device="cuda")
    d = torch.zeros(65, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    p = [Xd.data_ptr(), 65, 17, Cd.data_ptr(), 16, None, out.data_ptr(), d.data_ptr(), None, s]
    for i, bad in ((0, None), (1, 1 << 31), (2, 0), (3, None), (6, None), (7, None),
                   (8, out.data_ptr())):                # (changed without prev)
        assert L.dmlp_kmeans_assign(*(p[:i] + [bad] + p[i + 1:])) == -1, i
    assert L.dmlp_kmeans_assign(*(p[:4] + [0] + p[5:])) == 0
    assert L.dmlp_cluster_sums_bytes(-1, 4, 17) == -1
    torch.cuda.synchronize()
    assert (out == -5).all()
