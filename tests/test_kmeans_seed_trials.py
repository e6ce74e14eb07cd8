"""GPU tier of the greedy seeding (csrc/kmeans_seed.hip) through ops.knn and KMeans — against
tests/helpers/kmeans_seed_trials_contract.py and the CPU twin, bit for bit."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.models import KMeans
from distributed_machine_learning_project_amd.ops import knn as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import kmeans_seed_contract as SC  # noqa: E402
import kmeans_seed_trials_contract as TC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch


@pytest.mark.parametrize("case", TC.CASES, ids=str)
def test_trials(torch_cuda, case):
    X, i0, u, ref = TC.trials_case(*case)
    Xd = torch_cuda.from_numpy(X).cuda()
    runs = [K.kmeans_seed_gpu(Xd, case[2], i0, u) for _ in range(2)]
    cpu = K.kmeans_seed_cpu(X, case[2], i0, u)
    for got in runs:                                    # (the second call: the same bits)
        got = [t.cpu().numpy() for t in got]
        TC.check(got, ref)
        TC.check(got, cpu)


def test_kmeans_greedy(torch_cuda):
    X, Kc, seed, _ = SC.model_case()
    km = KMeans(Kc, seed, device="gpu", seeding="greedy").fit(X)
    cpu = KMeans(Kc, seed, device="cpu", seeding="greedy").fit(X)
    np.testing.assert_array_equal(km.seed_rows_, cpu.seed_rows_)
    np.testing.assert_array_equal(SC.bits(km.cluster_centers_), SC.bits(cpu.cluster_centers_))
    assert (km.n_iter_, SC.bits(km.inertia_)) == (cpu.n_iter_, SC.bits(cpu.inertia_))


def test_trials_arguments(torch_cuda):
    """-1 before any launch for what dmlp.h lists, outputs untouched; N = 0, K = 0: no launch"""
    torch, L = torch_cuda, _lib.lib()
    X, i0, u, _ = TC.trials_case(65, 33, 9, 4, "int")
    Xd, ud = torch.from_numpy(X).cuda(), torch.from_numpy(u).cuda()
    seeds = torch.full((9,), -5, dtype=torch.int32, device="cuda")
    C = torch.full((9, 33), 7.0, dtype=torch.float64, device="cuda")
    w = torch.full((65,), 7.0, dtype=torch.float64, device="cuda")
    nbytes = L.dmlp_kmeans_seed_trials_bytes(65, 33, 4)
    # m, R, B, the candidate rows, then 1 + 4 words in whole doubles
    assert nbytes == 8 * (4 * 65 + 4 * 2 + 4 * 1 + 4 * 33 + 3)
    assert {L.dmlp_kmeans_seed_trials_bytes(*b) for b in ((1 << 31, 33, 4), (65, 0, 4), (65, 33, 0),
                                                          (65, 33, 17))} == {-1}
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    p = [Xd.data_ptr(), 65, 33, 9, 4, i0, ud.data_ptr(), seeds.data_ptr(), C.data_ptr(),
         w.data_ptr(), ws.data_ptr(), nbytes, s]
    for i, bad in ((0, None), (1, 1 << 31), (2, 0), (4, 0), (4, 17), (5, 65), (5, -1), (6, None),
                   (7, None), (8, None), (9, None), (10, None), (11, nbytes - 1)):
        assert L.dmlp_kmeans_seed_trials(*(p[:i] + [bad] + p[i + 1:])) == -1, i
    for i in (1, 3):
        assert L.dmlp_kmeans_seed_trials(*(p[:i] + [0] + p[i + 1:])) == 0
    torch.cuda.synchronize()
    assert (seeds == -5).all() and (C == 7.0).all() and (w == 7.0).all()
