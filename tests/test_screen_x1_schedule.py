"""The single-term screen's step schedule at the ends of the scan and at slice boundaries.

k_screen_x1 (csrc/screen_x1.hip) runs its epilogue one step behind its MFMAs, in a ring of 4
steps whose accumulators and pair maxima start at -inf, and judges the last step after the loop.
A schedule change can only go wrong where the scan starts, where it ends and where a slice ends,
so the shapes here are the smallest that have those: N = 64, 100, 130, 300 (1, 2, 3 and 5 tiles:
4, 8, 12 and 20 steps, with padded rows at 100, 130 and 300), Q = 1, 64, 70 (one lane, a full
wave, a second workgroup of 6 columns), on the generator's uniform data and on planted data whose
best 8 rows are rows 0 - 7 (the first pair of steps) for half of the queries and the last 8 real
rows (the last pair) for the others; half of the planted queries ask for exactly those 8.

The GPU cases call the C ABI and check what the kernels wrote — invariants I1 - I5 of
tests/test_screen_contract.py (its check_lists and runners, imported), every count >= 0 — against
the float64 reference of tests/helpers/x1_contract.py; the CPU case shows that the reference's own
screen model satisfies I2 - I4 at every shape, so a failing GPU case is not the helper's fault.

The early-start cases preset every ready word with per-tile max norms that increase strictly.
With the last word set the kernel takes the whole image at once (widen() in screen_x1.hip), so
its eps folds every tile's norm before the first step instead of growing at each tile boundary:
the cases check the final eps (I1) and the lists, and that no wave waited or timed out.
"""
import functools
import os
import sys

import numpy as np
import pytest

import distributed_machine_learning_project_amd as dmlp
from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.ops import knn as K

HERE = os.path.dirname(os.path.abspath(__file__))
for _d in (HERE, os.path.join(HERE, "helpers")):
    if _d not in sys.path:
        sys.path.insert(0, _d)
import test_screen_contract as TSC  # noqa: E402  (Ops, the runners, check_lists: I1 - I5)
import x1_contract as X1  # noqa: E402

NS = (64, 100, 130, 300)
QS = (1, 64, 70)
KMAXS = (16, 48)   # 16: the 16-entry pair screen; 48: the 32-entry screen
KINDS = ("uniform", "planted", "growth")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch


def _q6(x):
    """6 decimals, as the input text carries them"""
    return np.rint(np.asarray(x) * 1.0e6) / 1.0e6


@functools.lru_cache(maxsize=None)
def case(kind: str, N: int, Q: int, A: int, kmax: int):
    """(input, reference), built once per shape and shared (never modified)."""
    seed = 1000 * N + 10 * Q + A + kmax
    inp = dmlp.generate(N, Q, A, 0.0, 1000.0, 1, kmax, 10, seed=seed)
    X, Qx, k = inp.X.copy(), inp.Qx.copy(), inp.k.copy()
    g = np.random.default_rng(seed + 1)
    if kind == "planted":
        # two clusters of 8 rows, 1 wide, among rows hundreds away: rows 0 - 7 and the last 8 real
        # rows; query q sits in cluster (q + Q) & 1 (Q = 1: the last pair) and asks for exactly the
        # cluster (k = 8) or for kmax neighbours, the cluster first
        cen = np.stack([np.full(A, 250.0), np.full(A, 750.0)])
        X[:8] = _q6(cen[0] + g.uniform(-1.0, 1.0, (8, A)))
        X[N - 8:] = _q6(cen[1] + g.uniform(-1.0, 1.0, (8, A)))
        which = (np.arange(Q) + Q) & 1
        Qx = _q6(cen[which] + g.uniform(-0.5, 0.5, (Q, A)))
        k = np.where((np.arange(Q) >> 1) & 1, min(kmax, N), 8).astype(np.int32)
    elif kind == "growth":
        # the rows of tile t spread 2^t times wider around the centre: per-tile max norms that
        # increase strictly (asserted where the ready words are made)
        amp = 10.0 * 2.0 ** (np.arange(N) // 64)
        X = _q6(500.0 + (g.uniform(-1.0, 1.0, (N, A)) * amp[:, None]))
        Qx = _q6(500.0 + g.uniform(-1.0, 1.0, (Q, A)) * amp.max())
    else:
        assert kind == "uniform"
    inp = type(inp)(inp.labels, np.ascontiguousarray(X), k, np.ascontiguousarray(Qx))
    ref = X1.reference(inp.X, inp.Qx, inp.k, hl=1)
    if kind == "planted":
        for q in range(Q):
            want = range(8) if which[q] == 0 else range(N - 8, N)
            assert sorted(ref.nn_i[q, :8].tolist()) == list(want), "the planted rows must be the best 8"
    return inp, ref


def shapes():
    """every (kind, N, Q, A, kmax) of the plain-screen cases: A = 32 in full, KT 2 once per class"""
    out = [(kind, N, Q, 32, kmax) for kind in ("uniform", "planted") for N in NS for Q in QS
           for kmax in KMAXS]
    return out + [("uniform", 130, 70, 64, kmax) for kmax in KMAXS]


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def grows_for(ref, kmax):
    """rows per group entry of the screen that serves (KT, kmax) (dmlp.h; test_screen_contract's
    grows_of asserts the same of the library on the GPU tier)"""
    return 8 if kmax <= 32 or ref.KT == 1 else 4


def cap_for(kmax):
    return 4 * ((16 if kmax <= 32 else 32) - 1)


def no_overflow(ls, ctx):
    cnt = ls.host()[1]
    assert (cnt != -1).all() and (cnt >= 0).all(), f"{ctx}: counts {np.unique(cnt).tolist()}"


# ------------------------------------------------------------------ CPU: the reference itself
class ModelLists:
    """The lists the screen's arithmetic gives without the MFMA's fp32 accumulation order: group
    maxima of fp32(a_model) floored to 16-bit keys, ak the k-th largest key of the slice's groups
    (when it has k of them; else no threshold), h = ak - 2 eps, every group whose key reaches
    key(h) listed as key << 16 | group index.
    rows: the query list (list position p holds the lists of reference row rows[p]; None: every
    row in order).  eps_rows / k_rows: the rows eps and k are taken from (default rows; anything
    else models a kernel that indexes them wrongly).  k: the k per row (default ref.k).
    slack_keys: list down to that many 16-bit keys below key(h) (what a threshold lower by the
    fp32 accumulation order's difference could add: how full the real lists can get)."""

    def __init__(self, ref, S, cap, grows, rows=None, eps_rows=None, k_rows=None, k=None,
                 slack_keys=0):
        self.S, self.cap = S, cap
        rows = np.arange(ref.Q) if rows is None else np.asarray(rows, np.int64)
        eps_of = ref.eps[rows if eps_rows is None else np.asarray(eps_rows, np.int64)]
        k_of = np.asarray(ref.k if k is None else k)[rows if k_rows is None
                                                     else np.asarray(k_rows, np.int64)]
        Q = self.nq = len(rows)
        self.ids = np.zeros((Q, S, cap), np.int64)
        self.cnt = np.zeros((Q, S), np.int32)
        self.h = np.zeros((Q, S, 2), np.float32)
        tps = X1.tiles_per_slice(ref.n_tiles, S)
        lowest = np.float32(-np.finfo(np.float32).max)
        for s in range(S):
            r0, r1 = X1.slice_rows(ref.n_tiles, S, s, ref.N)
            nts = max(0, min((s + 1) * tps, ref.n_tiles) - s * tps)
            gm = X1.group_max(ref.a_model[rows][:, r0:r1].astype(np.float32), nts, grows)
            for p in range(Q):
                real = np.nonzero(gm[p] > -np.inf)[0]
                keys = X1.key16(gm[p, real])
                kq, h = int(k_of[p]), lowest
                if 1 <= kq <= len(real):
                    ak = np.float32(X1.decode16(np.sort(keys)[-kq]))
                    h = max(lowest, np.float32(ak - np.float32(2.0) * eps_of[p]))
                keep = keys >= X1.key16(np.array([h], np.float32))[0] - slack_keys
                n = int(keep.sum())
                assert n <= cap
                self.ids[p, s, :n] = (keys[keep] << 16) | real[keep]
                self.cnt[p, s] = n
                self.h[p, s] = (h, eps_of[p])

    def host(self):
        return self.ids, self.cnt, self.h


@pytest.mark.parametrize("shape", shapes() + [("growth", N, Q, 32, kmax) for N in NS for Q in QS
                                              for kmax in KMAXS], ids=_id)
def test_reference_model_satisfies_invariants(shape):
    """I2 - I4 (and I1, I5 trivially) hold for the float64 reference's own screen model at every
    shape of this file, one slice and two."""
    kind, N, Q, A, kmax = shape
    _, ref = case(*shape)
    grows = grows_for(ref, kmax)
    for S in (1, 2):
        ls = ModelLists(ref, S, cap_for(kmax), grows)
        TSC.check_lists(ref, ls, grows, ctx=f"model {_id(shape)} S={S}")
        no_overflow(ls, f"model {_id(shape)} S={S}")


# ------------------------------------------------------------------ GPU: the plain screen
@pytest.mark.gpu
@pytest.mark.parametrize("shape", shapes(), ids=_id)
def test_x1_scan_ends(torch_cuda, shape):
    """dmlp_screen_x1 with one slice and with two (N = 64: the second slice is empty)."""
    kind, N, Q, A, kmax = shape
    inp, ref = case(*shape)
    ops = TSC.Ops(torch_cuda, ref, inp.labels)
    grows = TSC.grows_of(ops.L, ref, kmax)
    assert grows == grows_for(ref, kmax)
    for S in (1, 2):
        ctx = f"{_id(shape)} S={S}"
        ls = TSC.run_x1(ops, kmax, S)
        assert ls.cap == cap_for(kmax)
        TSC.check_lists(ref, ls, grows, ctx=ctx)
        no_overflow(ls, ctx)


# ------------------------------------------------------------------ GPU: early start
@pytest.mark.gpu
@pytest.mark.parametrize("kmax", KMAXS)
@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("N", NS)
def test_x1_early_tile_slices(torch_cuda, N, Q, kmax):
    """dmlp_screen_x1_early with one ready word per tile, every word preset, the tiles' max norms
    increasing strictly: the lists satisfy I1 - I5 with the whole image's eps."""
    inp, ref = case("growth", N, Q, 32, kmax)
    bits = TSC.ready_words(ref, 1)
    assert len(bits) == ref.n_tiles and (np.diff(bits.view(np.float32)) > 0).all()
    ops = TSC.Ops(torch_cuda, ref, inp.labels)
    ls, estats = TSC.run_x1_early(ops, kmax, rdy_tiles=1)
    ctx = f"early N={N} Q={Q} kmax={kmax}"
    assert estats[0] == 0 and estats[2] == 0, f"{ctx}: waits {estats[0]}, timeouts {estats[2]}"
    TSC.check_lists(ref, ls, TSC.grows_of(ops.L, ref, kmax), ctx=ctx)
    no_overflow(ls, ctx)
    # the same lists as the plain screen's over the landed image
    plain = TSC.run_x1(ops, kmax, 1)
    (i0, c0, h0), (i1, c1, h1) = plain.host(), ls.host()
    np.testing.assert_array_equal(c1, c0)
    np.testing.assert_array_equal(h1, h0)
    live = np.arange(ls.cap).reshape(1, 1, -1) < c0[:, :, None]
    np.testing.assert_array_equal(np.where(live, i1, 0), np.where(live, i0, 0))


# ------------------------------------------------------------------ GPU: two passes
@pytest.mark.gpu
@pytest.mark.parametrize("Q", QS)
def test_x1_two_pass_small(torch_cuda, Q):
    """N = 300, k = 33: k' = 7 over S1 = 5 one-tile slices (S1 k' >= k; the last slice's 44 rows
    make 7 pair groups, so every slice forms a threshold), dmlp_x1_seed, then
    dmlp_screen_x1_collect over 2 slices of 3 and 2 tiles (12 and 8 steps)."""
    torch = torch_cuda
    N, A, k, S1, S2, ccap = 300, 32, 33, 5, 2, 256
    inp = dmlp.generate(N, Q, A, 0.0, 1000.0, k, k, 10, seed=7 + Q)
    ref = X1.reference(inp.X, inp.Qx, inp.k, hl=1)
    ops = TSC.Ops(torch, ref, inp.labels)
    L, p = ops.L, TSC._p
    kp = np.full(Q, (k + S1 - 1) // S1, np.int32)
    ctx = f"two-pass N={N} Q={Q}"
    first = TSC.run_x1(ops, int(kp.max()), S1, qk=torch.from_numpy(kp).cuda())
    TSC.check_lists(ref, first, TSC.grows_of(L, ref, int(kp.max())), k=kp, ctx=ctx + " first pass")
    no_overflow(first, ctx + " first pass")
    hseed = torch.full((Q,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(L.dmlp_x1_seed(p(first.h), p(first.cnt), S1, Q, p(hseed), TSC._stream(torch)),
               "x1_seed")
    ls = TSC.Lists(torch, Q, S2, ccap)
    _lib.check(L.dmlp_screen_x1_collect(
        ref.KT, A, p(ops.xfrag), p(ops.xinit), ref.n_tiles, N, p(ops.qhi), p(ops.qn), p(ops.qidx),
        p(ops.qk), Q, ops.xnmax, ops.bad, p(hseed), ccap, S2, p(ls.ids), p(ls.cnt), p(ls.h),
        TSC._stream(torch)), "screen_x1_collect")
    torch.cuda.synchronize()
    hs = hseed.cpu().numpy().astype(np.float64)
    eps = ref.eps.astype(np.float64)
    for q in range(Q):
        t = np.partition(ref.a_exact[q], -k)[-k]
        slack = 2.0 ** -22 * max(abs(hs[q]), abs(t), eps[q])
        assert hs[q] <= t - eps[q] + slack, f"{ctx}: seed of query {q} above t - eps"
    TSC.check_lists(ref, ls, 4, ctx=ctx + " collect", thresholds=False)
    no_overflow(ls, ctx + " collect")
    TSC.refine_groups(ops, ls, k, ctx, collect=1)


# ------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
@pytest.mark.parametrize("N", NS)
def test_step_end_to_end(torch_cuda, N):
    """K.step on the planted data: ids, distances, labels and checksums equal the CPU oracle's,
    bit for bit."""
    inp, ref = case("planted", N, 70, 32, 16)
    r = K.step(inp.X, inp.labels, (0, 10), inp.Qx, inp.k, lists=True)
    torch_cuda.cuda.synchronize()
    d, i = r.dist.cpu().numpy(), r.ids.cpu().numpy()
    for q in range(ref.Q):
        kq = int(inp.k[q])
        np.testing.assert_array_equal(i[q, :kq], ref.nn_i[q, :kq], err_msg=f"N={N} ids q={q}")
        np.testing.assert_array_equal(d[q, :kq], ref.nn_d[q, :kq], err_msg=f"N={N} dist q={q}")
    lab_ref, cs_ref = K.finalize_cpu(ref.nn_i, inp.k, inp.labels)
    np.testing.assert_array_equal(r.label.cpu().numpy(), lab_ref)
    np.testing.assert_array_equal(r.checksum.cpu().numpy().view(np.uint64), cs_ref)
