"""What the screened k-means assignment (csrc/kmeans_screen.hip) leaves BEHIND its result, on the
GPU: the row operands of k_kmeans_rows, every row's candidate list, the escalation list and the
stats, against the float64 model of tests/helpers/kmeans_screen_contract.py — next to the exact
label / dmin / changed.  test_kmeans_screen_model.py shows on the CPU what each input family
stresses; the lists are read through dmlp_kmeans_screen_layout.

Each case calls dmlp_kmeans_screen_prep_rows once and dmlp_kmeans_assign_screened twice in a row
with its own workspace, then reads everything back."""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.models import KMeans, NearestCentroid
from distributed_machine_learning_project_amd.ops import knn as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import kmeans_contract as KC  # noqa: E402
import kmeans_screen_contract as S  # noqa: E402

pytestmark = pytest.mark.gpu
ids = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def prep_rows(torch, X):
    """(device rows X, the row handle's bytes) of dmlp_kmeans_screen_prep_rows"""
    L = _lib.lib()
    N, A = X.shape
    Xd = dev(torch, X)
    rows = torch.zeros(L.dmlp_kmeans_screen_rows_bytes(N, A), dtype=torch.uint8, device="cuda")
    assert L.dmlp_kmeans_screen_prep_rows(Xd.data_ptr(), N, A, rows.data_ptr(), rows.numel(),
                                          torch.cuda.current_stream().cuda_stream) == 0
    return Xd, rows


def assign_twice(torch, Xd, rows, Cn, prev):
    """two calls in a row on one workspace -> the second call's label, dmin, changed, stats, the
    max-norm word, cnt, esc, cand (the first call's result is checked to be the same)"""
    L = _lib.lib()
    N, A = Xd.shape
    Kc = Cn.shape[0]
    Cd, pd = dev(torch, Cn), dev(torch, prev)
    ws = torch.zeros(L.dmlp_kmeans_screen_bytes(N, A, Kc), dtype=torch.uint8, device="cuda")
    _, (o_cnt, o_esc, o_cand) = S.layout(N, A, Kc)
    out = []
    for _ in range(2):
        label = torch.full((N,), -5, dtype=torch.int32, device="cuda")
        dmin = torch.zeros(N, dtype=torch.float64, device="cuda")
        changed = torch.full((1,), -5, dtype=torch.int32, device="cuda")
        stats = torch.full((2,), -5, dtype=torch.int32, device="cuda")
        assert L.dmlp_kmeans_assign_screened(
            rows.data_ptr(), rows.numel(), Xd.data_ptr(), N, A, Cd.data_ptr(), Kc, pd.data_ptr(),
            label.data_ptr(), dmin.data_ptr(), changed.data_ptr(), stats.data_ptr(),
            ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        w = ws.cpu().numpy()
        out.append(dict(
            label=label.cpu().numpy(), dmin=dmin.cpu().numpy(), changed=int(changed[0]),
            stats=stats.cpu().numpy(), word=w[:4].view(np.float32)[0],
            cnt=w[o_cnt:o_cnt + 4 * N].view(np.int32).copy(),
            esc=w[o_esc:o_esc + 4 * N].view(np.int32).copy(),
            cand=w[o_cand:o_cand + 64 * N].view(np.int32).reshape(N, 16).copy()))
    a, b = out
    np.testing.assert_array_equal(a["label"], b["label"])
    np.testing.assert_array_equal(KC.bits(a["dmin"]), KC.bits(b["dmin"]))
    assert a["changed"] == b["changed"] and tuple(a["stats"]) == tuple(b["stats"])
    return b


def check_result(case, got):
    m = case.m
    cpu = K.kmeans_assign_cpu(case.X, case.Cn, case.prev)
    for label, dmin, ndiff in ((m.label, m.dmin, case.ndiff), cpu):
        np.testing.assert_array_equal(got["label"], label)
        np.testing.assert_array_equal(KC.bits(got["dmin"]), KC.bits(dmin))
        assert got["changed"] == ndiff


def check_rows(case, rows):
    """mu, the bf16 words (zero past A, KT = 3 as 3 x 4 words), |x'|^2 and the +inf marks;
    returns the device's xn"""
    m = case.m
    N, A = m.N, m.A
    KT = (A + 31) // 32
    (o_hi, o_xn), _ = S.layout(N, A, 1)
    r = rows.cpu().numpy()
    mu = r[:8 * A].view(np.float64)
    fin = ~np.isnan(m.mu)      # (a NaN's sign and payload are not part of the contract)
    np.testing.assert_array_equal(KC.bits(mu[fin]), KC.bits(m.mu[fin]))
    assert np.isnan(mu[~fin]).all()
    assert o_xn - o_hi == (N * KT * 64 + 255) // 256 * 256   # no pad to 4 fragments at KT = 3
    hi = r[o_hi:o_hi + N * KT * 64].view(np.uint16).reshape(N, KT * 32)
    np.testing.assert_array_equal(hi, m.hi_bits)
    assert not hi[:, A:].any()
    xn = r[o_xn:o_xn + 4 * N].view(np.float32).copy()
    np.testing.assert_array_equal(np.isinf(xn), m.row_bad)
    ok = ~m.row_bad
    near = (xn[ok] == m.xn[ok]) | (xn[ok] == np.nextafter(m.xn[ok], np.float32(np.inf))) | \
        (xn[ok] == np.nextafter(m.xn[ok], np.float32(-np.inf)))
    assert near.all(), "xn is more than one fp32 ulp from fp32(sum (x - mu)^2)"
    return xn


def check_lists(case, got, xn):
    """the per-row lists, the escalation list and the stats against must / may with eps
    recomputed from the xn and the max-norm word the device wrote; returns the row classes"""
    m = case.m
    N, Kc = m.N, m.K
    if not m.cbad:   # the max-norm word: rounded up, by no more than prep.hip's 1e-6
        assert m.cn_max <= float(got["word"]) <= float(m.cm) * (1.0 + 1.0e-6)
    may, cls = S.sets_of(m, S.eps_of(m.A, xn, got["word"]))
    cnt, cand = got["cnt"], got["cand"]
    escalated = cnt == -1
    assert ((cnt == -1) | ((cnt >= 1) & (cnt <= S.SLOTS))).all()
    assert escalated[cls == S.MUST_ESC].all(), "a row that must escalate has a list"
    assert not escalated[cls == S.MUST_NOT].any(), "a row whose may set fits was escalated"
    for i in np.flatnonzero(~escalated):
        lst = cand[i, :cnt[i]]
        assert (np.diff(lst) > 0).all() and lst[0] >= 0 and lst[-1] < Kc, (i, lst)
        assert np.isin(np.flatnonzero(m.must[i]), lst).all(), \
            (i, "the list lost", np.flatnonzero(m.must[i]), lst)
        assert may[i, lst].all(), (i, "outside may", lst[~may[i, lst]])
    nesc = int(escalated.sum())
    assert got["stats"][0] == nesc
    assert sorted(got["esc"][:nesc]) == list(np.flatnonzero(escalated))
    assert got["stats"][1] == cnt[~escalated].sum()
    return cls, cnt


def run_case(torch, case):
    Xd, rows = prep_rows(torch, case.X)
    got = assign_twice(torch, Xd, rows, case.Cn, case.prev)
    check_result(case, got)
    xn = check_rows(case, rows)
    cls, cnt = check_lists(case, got, xn)
    print(f"{case.name} A={case.m.A} K={case.m.K}: escalated {got['stats'][0]}, candidates "
          f"{got['stats'][1]}, longest list {cnt.max()}, classes {np.bincount(cls, minlength=3)}")
    return got, cls, cnt


AK = list(S.SHAPES.items())


@pytest.mark.parametrize("A,Kc", AK + [(17, 300)] + [(128, f"tile{i}") for i in range(4)],
                         ids=ids)
def test_neartie(torch_cuda, A, Kc):
    """winners in late slots; hits over registers, kg lanes, steps and LDS tiles; tile0 .. 3:
    K = T, T + 1, 2 T, 2 T + 1 at A = 128"""
    if isinstance(Kc, str):
        A, Kc = S.tile_shapes()[int(Kc[4:])]
    got, cls, cnt = run_case(torch_cuda, S.neartie(A, Kc))
    assert got["stats"][0] == 0


@pytest.mark.parametrize("A,Kc", AK, ids=ids)
def test_offset(torch_cuda, A, Kc):
    got, _, _ = run_case(torch_cuda, S.offset(A, Kc))
    assert got["stats"][0] == 0


@pytest.mark.parametrize("A,Kc", AK, ids=ids)
def test_coherent(torch_cuda, A, Kc):
    """every bf16 rounding of one sign: the list must still hold the low-scoring tie"""
    got, _, _ = run_case(torch_cuda, S.coherent(A, Kc))
    assert got["stats"][0] == 0


@pytest.mark.parametrize("A", list(S.SHAPES))
def test_far(torch_cuda, A):
    run_case(torch_cuda, S.far(A))


@pytest.mark.parametrize("e", S.TINY_E)
@pytest.mark.parametrize("Kc", S.TINY_K)
@pytest.mark.parametrize("A", list(S.SHAPES))
def test_tiny(torch_cuda, A, Kc, e):
    run_case(torch_cuda, S.tiny(A, Kc, e))


@pytest.mark.parametrize("nonfinite", [False, True], ids=["finite", "nonfinite"])
@pytest.mark.parametrize("A,Kc", AK, ids=ids)
def test_mixed(torch_cuda, A, Kc, nonfinite):
    """escalating rows among rows that must not, prev over both: stats, cnt and esc exactly"""
    case = S.mixed(A, Kc, nonfinite)
    got, cls, cnt = run_case(torch_cuda, case)
    assert not (cls == S.FREE).any()
    want = case.m.cls == S.MUST_ESC
    np.testing.assert_array_equal(cls == S.MUST_ESC, want)
    np.testing.assert_array_equal(cnt == -1, want)
    assert got["stats"][0] == want.sum() == (N_ESC if not nonfinite else case.m.N)
    np.testing.assert_array_equal(np.sort(got["esc"][:want.sum()]), np.flatnonzero(want))


N_ESC = int(S.mixed_escalates(np.arange(S.N_ROWS)).sum())


def test_row_handle_reuse(torch_cuda):
    """one row handle against neartie's centroids, then against the same centroids moved by 1e3
    and by 1e6 in every coordinate.  At 1e3 the model's may sets still fit (|c'|^2 / 2 separates
    the centroids faster than eps grows), so no row may escalate; at 1e6 every row's list
    overflows: the model keeps more than 16 centroids within ONE eps of the best score, and the
    fp32 accumulation that separates the kernel's score from the model's is below eps / 2."""
    torch = torch_cuda
    base = S.neartie(32, 1100)
    Xd, rows = prep_rows(torch, base.X)
    xn = check_rows(base, rows)
    for shift in (0.0, 1.0e3, 1.0e6):
        case = base if shift == 0.0 else S.neartie_shifted(32, 1100, shift)
        got = assign_twice(torch, Xd, rows, case.Cn, case.prev)
        check_result(case, got)
        check_lists(case, got, xn)
        if shift == 1.0e6:
            sure = S.keep_model(case.m, S.eps_of(32, xn, got["word"]), 0.5).sum(axis=1)
            assert sure.min() > S.SLOTS
            assert got["stats"][0] == case.m.N
        else:
            assert got["stats"][0] == 0


def blobs(N, A, seed):
    rng = np.random.default_rng(seed)
    return np.round(rng.normal(0, 1, (N, A)) + 6 * rng.integers(0, 3, (N, 1)), 3)


@pytest.mark.parametrize("Kc,screened", [(256, True), (255, False)])
def test_auto_switches_at_the_threshold(torch_cuda, monkeypatch, Kc, screened):
    """assign="auto" (the default) takes the screen from 256 centroids on, on both estimators"""
    calls = []
    real = K.kmeans_rows_gpu
    monkeypatch.setattr(K, "kmeans_rows_gpu", lambda X: calls.append(X.shape) or real(X))
    X = blobs(300, 2, 5)
    km = KMeans(Kc, "first", device="gpu").fit(X)
    cpu = KMeans(Kc, "first", device="cpu").fit(X)
    assert bool(calls) == screened
    np.testing.assert_array_equal(KC.bits(km.cluster_centers_), KC.bits(cpu.cluster_centers_))
    np.testing.assert_array_equal(km.labels_, cpu.labels_)
    assert (km.n_iter_, KC.bits(km.inertia_)) == (cpu.n_iter_, KC.bits(cpu.inertia_))
    del calls[:]
    y = np.arange(300) % Kc
    Q = blobs(40, 2, 6)
    got = NearestCentroid(device="gpu").fit(X, y).predict(Q)
    assert bool(calls) == screened
    np.testing.assert_array_equal(got, NearestCentroid(device="cpu").fit(X, y).predict(Q))
