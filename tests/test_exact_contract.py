"""Kernel-level contract of the exact tier and the K4 merge, through the C ABI.

The dispatcher (local.h exact_pass) sorts its query list, passes kstride == kmax into pre-filled
outputs, takes workspaces from grow-only arenas and re-runs whatever the fp64 screen hands back,
so a false overflow, a write past k_q, into a row that is not listed or past the workspace never
shows through it.  Here every exact entry point of dmlp.h is called directly on an unsorted
subset of the rows, into outputs and workspaces with sentinel bands around them
(tests/helpers/result_contract.py: guarded), and every slot is compared with the float64
reference of that helper or must still hold its sentinel.  All comparisons are bit-exact.

The untouched-slot rules, from dmlp.h:
  dmlp_exact_topk, dmlp_fallback_select, dmlp_fallback_topk
      write slots [0, min(k_q, N)) of the listed rows and nothing else
  dmlp_exact_f64
      listed rows with status 0: [0, min(k_q, N)) the list, [min(k_q, N), kstride) = (+inf, -1);
      listed rows with status 1: [0, k_q) untouched, [k_q, kstride) = (+inf, -1) (the shared
      refine pads every listed row before it looks at the candidates)
  dmlp_merge
      writes every slot of [0, kout) of every row
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import refine_contract as RF  # noqa: E402
import result_contract as RC  # noqa: E402
import x1_contract as X1  # noqa: E402

pytestmark = pytest.mark.gpu

NEAR_TIE_P = 160     # tests/test_result_contract_model.py shows what this input discriminates


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


# ------------------------------------------------------------------ inputs (built once, shared)
@functools.lru_cache(maxsize=None)
def data(kind: str, N: int, A: int, Q: int):
    """(X [N, A], Qx [Q, A], D [Q, N]): D the left-to-right reference distances.
    uniform: 6-decimal values in [0, 1000); query 2 equals a data row (distance +0.0).
    equal:   every row 2.0; even queries 0.0, odd queries 2.0 (every distance +0.0).
    huge:    uniform with 1e200 in three rows: real neighbours at distance +inf, which order by
             id descending once k reaches them.
    span:    A = 1, x = 10^u, u in [-6, 6], queries 0: distances from 1e-12 to 1e12.
    near:    near_tie_input (N = 2000 + 160, Q = 5)."""
    rng = np.random.default_rng(N * 131 + A * 7 + Q)
    if kind == "near":
        X, Qx, _ = RC.near_tie_input(A, NEAR_TIE_P)
        assert X.shape[0] == N and Qx.shape[0] == Q
    elif kind == "equal":
        X = np.full((N, A), 2.0)
        Qx = np.zeros((Q, A))
        Qx[1::2] = 2.0
    elif kind == "span":
        assert A == 1
        X = 10.0 ** rng.uniform(-6.0, 6.0, (N, 1))
        Qx = np.zeros((Q, 1))
    else:
        X = np.round(rng.uniform(0.0, 1000.0, (N, A)), 6)
        Qx = np.round(rng.uniform(0.0, 1000.0, (Q, A)), 6)
        if Q > 2:
            Qx[2] = X[N // 3]
        if kind == "huge":
            for r in {1 % N, N // 2, N - 1}:
                X[r, A // 2] = 1e200
    X, Qx = np.ascontiguousarray(X), np.ascontiguousarray(Qx)
    D = np.stack([RC.dist_l2r(q, X) for q in Qx])
    return X, Qx, D


def subset(Q: int, nb: int, seed: int = 0, first=()):
    """nb distinct rows of [0, Q) in an unsorted order that starts Q - 1, 3, 0, 17, ... (after the
    rows of `first`)"""
    assert nb <= Q
    head = [r for r in (*first, Q - 1, 3, 0, 17) if 0 <= r < Q]
    head = list(dict.fromkeys(head))
    rest = [r for r in np.random.default_rng(seed + Q).permutation(Q) if r not in head]
    return np.array((head + rest)[:nb], np.int32)


def mixed_k(Q: int, kmax: int, seed: int = 0, kmin: int = 0):
    """k per row in [kmin, kmax], the ends and 1 included, mixed inside every workgroup."""
    k = np.random.default_rng(seed + kmax).integers(kmin, kmax + 1, Q).astype(np.int32)
    pins = [kmax, max(kmin, 1), kmin, kmax]
    for j, v in enumerate(pins):
        if 4 * j < Q:
            k[4 * j] = v
    k[Q - 1] = kmax
    return k


class Outputs:
    """Guarded (dist, id) lists of Q rows with stride ks."""

    def __init__(self, torch, Q, ks):
        self.d = RC.guarded(torch, (Q, ks), torch.float64)
        self.i = RC.guarded(torch, (Q, ks), torch.int32)
        self.Q, self.ks = Q, ks

    def check(self, D, k, qidx, ctx, pad_from=None, written=None):
        """Rows of qidx (where written, default all): slots [0, min(k, N)) equal the reference;
        slots from pad_from[q] on (None: none) hold (+inf, -1); every other slot of the payload
        still holds its sentinel; both guard bands are intact."""
        self.d.check_guards(ctx + " dist")
        self.i.check_guards(ctx + " ids")
        d, i = self.d.host(), self.i.host()
        N = D.shape[1]
        keep = np.ones((self.Q, self.ks), bool)       # slots that must be untouched
        for q in qidx:
            kq = max(0, min(int(k[q]), N))
            if written is None or written[q]:
                rd, ri = RC.topk_ref(D[q], kq, kq)
                np.testing.assert_array_equal(i[q, :kq], ri, err_msg=f"{ctx}: ids row {q}")
                np.testing.assert_array_equal(d[q, :kq], rd, err_msg=f"{ctx}: dist row {q}")
                keep[q, :kq] = False
            if pad_from is not None:
                p0 = int(pad_from[q])
                assert (i[q, p0:] == -1).all() and np.isposinf(d[q, p0:]).all(), \
                    f"{ctx}: row {q} slots [{p0}, {self.ks}) are not (+inf, -1)"
                keep[q, p0:] = False
        self.d.untouched(keep, ctx + " dist")
        self.i.untouched(keep, ctx + " ids")


class Operands:
    def __init__(self, torch, X, Qx, k, qidx):
        self.X, self.Qx = _dev(torch, X), _dev(torch, Qx)
        self.k, self.qidx = _dev(torch, k.astype(np.int32)), _dev(torch, qidx.astype(np.int32))
        self.N, self.A = X.shape
        self.nb = len(qidx)


# ------------------------------------------------------------------ dmlp_exact_topk
# kmax class -> (queries per workgroup, points per tile, attributes per chunk, candidate slots)
TOPK_VARIANTS = {16: (64, 128, 16, 48), 32: (64, 128, 16, 64), 64: (64, 128, 16, 128),
                 256: (16, 256, 8, 384)}


def run_topk(torch, X, Qx, D, k, qidx, kmax, ctx):
    Q = len(Qx)
    op = Operands(torch, X, Qx, k, qidx)
    out = Outputs(torch, Q, kmax + 5)
    rc = _lib.lib().dmlp_exact_topk(op.X.data_ptr(), op.N, op.A, op.Qx.data_ptr(),
                                    op.qidx.data_ptr(), op.k.data_ptr(), op.nb, kmax,
                                    out.d.ptr(), out.i.ptr(), out.ks, _stream(torch))
    assert rc == 0, ctx
    out.check(D, k, qidx, ctx)


@pytest.mark.parametrize("kmax", [16, 32, 64, 256])
def test_exact_topk_boundaries(torch_cuda, kmax):
    """Workgroup, tile and attribute-chunk boundaries of every variant; k from 0 to kmax mixed in
    one workgroup; k > N clamped; huge rows at distance +inf."""
    big = kmax == 256
    Q = 20 if big else 70
    for N in ([255, 257, 700] if big else [1, 127, 129, 300]):
        for A in ([7, 9] if big else [1, 15, 17, 33]):
            kind = "huge" if (N, A) in ((300, 17), (257, 9)) else "uniform"
            X, Qx, D = data(kind, N, A, Q)
            for nb in ([15, 17] if big else [1, 63, 65]):
                k = mixed_k(Q, kmax, seed=N + A + nb)
                run_topk(torch_cuda, X, Qx, D, k, subset(Q, nb, N + A), kmax,
                         f"exact_topk kmax={kmax} {kind} N={N} A={A} nb={nb}")


@pytest.mark.parametrize("kmax", [16, 32, 64, 256])
def test_exact_topk_all_equal(torch_cuda, kmax):
    """Every distance equal and N several times the candidate buffer: every round appends and
    compacts, and the answer is the k largest ids."""
    Q = 20
    N = 5 * TOPK_VARIANTS[kmax][3] + 3
    X, Qx, D = data("equal", N, 3, Q)
    k = mixed_k(Q, kmax)
    qidx = subset(Q, 17)
    assert (RC.topk_ref(D[0], kmax)[1] == np.arange(N - 1, N - 1 - kmax, -1)).all()
    run_topk(torch_cuda, X, Qx, D, k, qidx, kmax, f"exact_topk all-equal kmax={kmax}")


@pytest.mark.parametrize("A", [5, 8, 16, 32, 64])
def test_exact_topk_near_tie(torch_cuda, A):
    """Neighbours whose fp64 distances differ only by the order of summation."""
    X, Qx, D = data("near", RC.N_FILL + NEAR_TIE_P, A, 5)
    for kmax in (16, 32, 64, 200):
        k = np.array([kmax, kmax, 1, kmax - 3, kmax], np.int32)
        run_topk(torch_cuda, X, Qx, D, k, np.array([4, 0, 2, 1], np.int32), kmax,
                 f"exact_topk near-tie A={A} kmax={kmax}")


def test_exact_topk_rejects_large_kmax(torch_cuda):
    """kmax = 257 returns -1 before any launch (exact.hip: the check follows the nb / N early
    out and precedes every use of the pointers)."""
    torch = torch_cuda
    X, Qx, D = data("uniform", 127, 15, 70)
    k = mixed_k(70, 16)
    qidx = subset(70, 5)
    op = Operands(torch, X, Qx, k, qidx)
    out = Outputs(torch, 70, 21)
    rc = _lib.lib().dmlp_exact_topk(op.X.data_ptr(), op.N, op.A, op.Qx.data_ptr(),
                                    op.qidx.data_ptr(), op.k.data_ptr(), op.nb, 257, out.d.ptr(),
                                    out.i.ptr(), out.ks, _stream(torch))
    assert rc == -1
    out.check(D, k, qidx, "kmax 257", written=np.zeros(70, bool))


# ------------------------------------------------------------------ dmlp_fallback_select / _topk
def run_fallback(torch, which, X, Qx, D, k, qidx, ctx, written=None):
    L = _lib.lib()
    Q, N = len(Qx), X.shape[0]
    op = Operands(torch, X, Qx, k, qidx)
    ks = int(min(int(k.max()), N)) + 5
    out = Outputs(torch, Q, ks)
    fn, nbytes = ((L.dmlp_fallback_select, L.dmlp_fallback_select_bytes) if which == "select"
                  else (L.dmlp_fallback_topk, L.dmlp_fallback_bytes))
    wb = int(nbytes(op.nb, N))
    ws = RC.guarded(torch, wb, torch.uint8)      # exactly the advertised bytes, a guard behind
    args = (op.X.data_ptr(), N, op.A, op.Qx.data_ptr(), op.qidx.data_ptr(), op.k.data_ptr(), op.nb,
            ws.ptr())
    tail = (out.d.ptr(), out.i.ptr(), ks, _stream(torch))
    assert fn(*args, wb - 1, *tail) == -3, f"{ctx}: a workspace one byte short"
    ws.untouched(np.ones(wb, bool), ctx + " short workspace")
    out.check(D, k, qidx, ctx + " short workspace", written=np.zeros(Q, bool))
    assert fn(*args, wb, *tail) == 0, ctx
    ws.check_guards(ctx + " workspace")
    out.check(D, k, qidx, ctx, written=written)


SELECT_KMAX = 2048


@pytest.mark.parametrize("N", [1, 255, 257, 2048, 2049, 5000])
def test_fallback_select(torch_cuda, N):
    """k in {1, 2047, 2048} (clamped to N) per row; rows whose clamped k is 2049 are skipped and
    stay untouched; a query equal to a point (distance +0.0); all-equal rows (min == max: no
    radix pass, the tie branch when N > 2048); distances from 1e-12 to 1e12."""
    assert _lib.lib().dmlp_fallback_select_kmax() == SELECT_KMAX
    Q = 9
    k = np.array([1, 2047, 2048, 2049, 2048, 1, 2047, 2049, 2048], np.int32)
    qidx = subset(Q, 7, N, first=(2,))     # row 2: the uniform query that equals a data row
    written = np.minimum(k, N) <= SELECT_KMAX
    assert N < 2049 or not written[qidx].all()
    for kind, A in (("uniform", 5), ("equal", 3), ("span", 1), ("huge", 4)):
        X, Qx, D = data(kind, N, A, Q)
        run_fallback(torch_cuda, "select", X, Qx, D, k, qidx, f"fallback_select {kind} N={N}",
                     written=written)


def test_fallback_topk(torch_cuda):
    """k in {2049, N, N + 7 (clamped)} and small k at N = 3000 on the same data."""
    N, Q = 3000, 8
    k = np.array([2049, N, N + 7, 1, 2500, 17, N, 2049], np.int32)
    for kind, A in (("uniform", 5), ("equal", 3), ("span", 1), ("huge", 4)):
        X, Qx, D = data(kind, N, A, Q)
        run_fallback(torch_cuda, "topk", X, Qx, D, k, subset(Q, 6), f"fallback_topk {kind}")


@pytest.mark.parametrize("A", [5, 8, 16, 32, 64])
def test_fallback_near_tie(torch_cuda, A):
    """Both fallbacks on neighbours whose distances differ only by the order of summation: the
    rows kernel must sum left to right, the select and the sort must keep (dist asc, id desc)."""
    N = RC.N_FILL + NEAR_TIE_P
    X, Qx, D = data("near", N, A, 5)
    qidx = np.array([4, 0, 2, 1], np.int32)
    run_fallback(torch_cuda, "select", X, Qx, D, np.array([16, 64, 1, 2048, 32], np.int32), qidx,
                 f"fallback_select near-tie A={A}")
    run_fallback(torch_cuda, "topk", X, Qx, D, np.array([2049, 64, N, 16, 2100], np.int32), qidx,
                 f"fallback_topk near-tie A={A}")


def test_fallback_topk_rejects_int32_overflow(torch_cuda):
    """nb * N > 2^31 - 1 returns -1: in dmlp_fallback_topk the check follows the nb / N early out
    and precedes the workspace query and every use of a pointer, so null pointers are safe."""
    L = _lib.lib()
    assert L.dmlp_fallback_topk(None, 3000, 5, None, None, None, 1 << 20, None, 0, None, None, 8,
                                _stream(torch_cuda)) == -1


# ------------------------------------------------------------------ dmlp_exact_rows
@pytest.mark.parametrize("kind,N,A,Q", [("near", RC.N_FILL + NEAR_TIE_P, 5, 5),
                                        ("near", RC.N_FILL + NEAR_TIE_P, 32, 5),
                                        ("near", RC.N_FILL + NEAR_TIE_P, 64, 5),
                                        ("uniform", 130, 17, 5), ("huge", 65, 33, 5)])
def test_exact_rows(torch_cuda, kind, N, A, Q):
    """D[i][n] == dist_l2r bit for bit; ldd = N + 3: the pad columns and the rows past nq stay
    untouched."""
    torch = torch_cuda
    X, Qx, D = data(kind, N, A, Q)
    dX, dQ = _dev(torch, X), _dev(torch, Qx)
    for nq in (1, 65):
        qidx = (np.arange(nq)[::-1] * 3 + 4) % Q        # unsorted, with repeats
        rows = RC.guarded(torch, (nq + 1, N + 3), torch.float64)
        dq = _dev(torch, qidx.astype(np.int32))
        rc = _lib.lib().dmlp_exact_rows(dX.data_ptr(), N, A, dQ.data_ptr(), dq.data_ptr(), nq,
                                        rows.ptr(), N + 3, _stream(torch))
        assert rc == 0
        ctx = f"exact_rows {kind} A={A} nq={nq}"
        rows.check_guards(ctx)
        np.testing.assert_array_equal(rows.host()[:nq, :N], D[qidx], err_msg=ctx)
        keep = np.ones((nq + 1, N + 3), bool)
        keep[:nq, :N] = False
        rows.untouched(keep, ctx)


# ------------------------------------------------------------------ dmlp_exact_f64
# k_refine<8, 1, true> (dmlp_refine_groups_exact): P = E * 64 member slots; more survivors hand
# the query back
REFINE_MEMBERS = 512


def f64_layout(N, A, nq, kmax):
    out = (C.c_int64 * 8)()
    _lib.lib().dmlp_exact_f64_layout(N, A, nq, kmax, out)
    keys = ("S", "tps", "idcap", "ids", "cnt", "h", "xnmax", "mu")
    return dict(zip(keys, [int(v) for v in out]))


def f64_refine_status(e_lists, cnt, h, k, N, tps):
    """The group refine's hand-back decision for one query, from the screen's lists (k_refine with
    rescore = 0): tests/helpers/refine_contract.py states the rule for every refine; here 4-row
    groups, no image (every member with row < N of a live group survives) and more than
    REFINE_MEMBERS survivors (or an overflowed slice) -> status 1."""
    return RF.refine_status(e_lists, cnt, h, k, N, tps, grows=4, capacity=REFINE_MEMBERS)


def run_f64(torch, X, Qx, D, k, qidx, kmax, ctx, expect=None):
    """dmlp_exact_f64 on rows qidx; expect: None, "none" (no query may overflow) or "all"."""
    L = _lib.lib()
    (N, A), Q, nq = X.shape, len(Qx), len(qidx)
    lay = f64_layout(N, A, nq, kmax)
    S, tps, idcap = lay["S"], lay["tps"], lay["idcap"]
    cape = idcap - 4                      # 4 (SUB - 2) of the 4 (SUB - 1) id slots
    wb = int(L.dmlp_exact_f64_bytes(N, A, nq, kmax))
    assert wb >= lay["h"] + nq * S * 8
    op = Operands(torch, X, Qx, k, qidx)
    out = Outputs(torch, Q, kmax + 5)
    ws = RC.guarded(torch, wb, torch.uint8)
    status = RC.guarded(torch, Q, torch.int32)
    ovf = RC.guarded(torch, 1, torch.int32, fill=5)
    args = (op.X.data_ptr(), N, A, op.Qx.data_ptr(), op.qidx.data_ptr(), op.k.data_ptr(), nq, kmax,
            out.d.ptr(), out.i.ptr(), out.ks, status.ptr(), ovf.ptr(), ws.ptr())
    assert L.dmlp_exact_f64(*args, wb - 1, _stream(torch)) == -1, f"{ctx}: short workspace"
    assert L.dmlp_exact_f64(*args, wb, _stream(torch)) == 0, ctx
    for g, name in ((ws, "workspace"), (status, "status"), (ovf, "ovf_count")):
        g.check_guards(f"{ctx} {name}")
    w = ws.host()

    def region(off, n, dt):
        return w[off:off + n * np.dtype(dt).itemsize].view(dt)
    ids = region(lay["ids"], nq * S * idcap, np.int32).reshape(nq, S, idcap)
    cnt = region(lay["cnt"], nq * S, np.int32).reshape(nq, S)
    h = region(lay["h"], nq * S * 2, np.float32).reshape(nq, S, 2)
    mu = region(lay["mu"], A, np.float64)
    assert ((cnt >= -1) & (cnt <= cape)).all(), f"{ctx}: a count outside [-1, {cape}]"

    # the screen's score of every 4-row group, in float64 (the centring as the kernel rounds it)
    n_tiles = (N + 63) // 64
    G = n_tiles * 16
    with np.errstate(over="ignore", invalid="ignore"):
        xp, qp = X - mu, Qx[qidx] - mu
        xn, qq = (xp * xp).sum(1), (qp * qp).sum(1)
        flagged = ~(qq < 1e30) | ~(xn.max() < 1e30)        # the kernel's "big" columns
        score = np.full((nq, G * 4), -np.inf)
        score[:, :N] = qp @ xp.T - 0.5 * xn[None, :]
        gkey = X1.key16(score.reshape(nq, G, 4).max(2).astype(np.float32))
    gs = tps * 16                                          # groups per slice

    st_want = np.zeros(Q, np.int32)
    for p, q in enumerate(qidx):
        where = f"{ctx}: query {q}"
        kq = min(int(k[q]), N)
        if flagged[p]:
            assert (cnt[p] == -1).all(), f"{where}: magnitudes past the key range must overflow"
            st_want[q] = 1
            continue
        nn = RC.topk_ref(D[q], kq)[1].astype(np.int64)
        for s in range(S):
            c = int(cnt[p, s])
            n_real = max(0, min(G, (s + 1) * gs) - s * gs)
            if c < 0:       # a slice overflows only when it holds more groups than fit
                assert n_real > cape, f"{where} slice {s}: overflow, {n_real} groups fit {cape}"
                continue
            gi = (ids[p, s, :c].view(np.uint32) & 0xffff).astype(np.int64)
            assert len(np.unique(gi)) == c and (gi < n_real).all(), f"{where} slice {s}: entries"
            mine = nn[(nn // 4 >= s * gs) & (nn // 4 < (s + 1) * gs)] // 4 - s * gs
            lost = np.setdiff1d(mine, gi)
            assert len(lost) == 0, f"{where} slice {s}: groups {lost.tolist()} of neighbours lost"
        st_want[q] = f64_refine_status(ids[p].view(np.uint32), cnt[p], h[p], int(k[q]), N, tps)

    # what the float64 scores alone say about the refine's survivors (keys within 2 units: the
    # fp32 rounding of a score, the 15-bit threshold search and the fp32 subtraction)
    nm_hi = np.zeros(nq, np.int64)
    nm_lo = np.zeros(nq, np.int64)
    real4 = np.clip(N - 4 * np.arange(G), 0, 4)
    xm = np.sqrt(xn.max())
    for p, q in enumerate(qidx):
        if flagged[p]:
            continue
        if S == 1 or not 1 <= k[q] <= G:
            # one slice (its threshold is the screen's own) or fewer groups than k: no model of
            # the threshold, but no more survivors than points
            nm_hi[p] = N
            continue
        qm = np.sqrt(qq[p])
        eps = (2.0 ** -20 * (0.5 * xm * xm + qm * xm + (qm + xm) ** 2) + 1e-30) * 1.001
        t16 = np.sort(gkey[p])[-int(k[q])]
        kh = int(X1.key16(np.float32(X1.decode16(t16) - 2.0 * eps)).ravel()[0])
        nm_hi[p] = real4[gkey[p] >= kh - 2].sum()
        nm_lo[p] = real4[gkey[p] >= kh + 2].sum()
    fits = gs <= cape
    if expect == "none":
        assert fits and (nm_hi <= REFINE_MEMBERS).all() and not flagged.any(), \
            f"{ctx}: the model does not exclude an overflow (survivors up to {nm_hi.max()})"
    if expect == "all":
        assert (flagged | (nm_lo > REFINE_MEMBERS)).all(), f"{ctx}: the model predicts no overflow"
    st = status.host()
    for p, q in enumerate(qidx):
        if fits and not flagged[p] and nm_hi[p] <= REFINE_MEMBERS:
            assert st[q] == 0, f"{ctx}: query {q} handed back, the model holds {nm_hi[p]} survivors"
        if flagged[p] or nm_lo[p] > REFINE_MEMBERS:
            assert st[q] == 1, f"{ctx}: query {q} not handed back"
    listed = np.zeros(Q, bool)
    listed[qidx] = True
    np.testing.assert_array_equal(st[listed], st_want[listed], err_msg=f"{ctx}: status")
    status.untouched(~listed, ctx + " status")
    assert int(ovf.host()[0]) == 5 + int(st_want[listed].sum()), f"{ctx}: *ovf_count is added to"
    pad_from = np.where(st_want == 1, k, np.minimum(k, N))
    out.check(D, k, qidx, ctx, pad_from=pad_from, written=st_want == 0)
    return st_want[qidx]


F64_SHAPES = [(17, 1, 16), (17, 65, 64), (63, 65, 17),      # (17, 65, 64): k > N, clamped
 (65, 130, 64), (1000, 65, 16), (1000, 130, 17),
              (2160, 130, 64), (2160, 65, 16)]


@pytest.mark.parametrize("A", [1, 5, 32, 37, 48, 64])
def test_exact_f64_contract(torch_cuda, A):
    """Every fragment-count class of A, N around the 16-point step and the 64-point tile, one to
    three query blocks, kmax on both sides of the sub-buffer switch (the layout says which).
    On this uniform wide-range data no query may overflow, and the float64 model alone must say
    so (expect="none") — except A = 1 at N = 2160: the scores q'x' - x'^2 / 2 of the few hundred
    points nearest to a query all fall into the 16-bit key bucket of q'^2 / 2 (relative width
    2^-7), more than the refine's 512 member slots for about half of the queries.  There the model
    decides query by query: handed back where it counts more than 512 survivors at keys two
    units above the threshold, answered where it counts at most 512 two units below it."""
    L = _lib.lib()
    assert L.dmlp_exact_f64_amax() == 64 and L.dmlp_exact_f64_kmax() == 64
    if A <= 32:
        assert f64_layout(1000, A, 65, 16)["idcap"] < f64_layout(1000, A, 65, 17)["idcap"]
    Q = 140
    for N, nq, kmax in F64_SHAPES:
        X, Qx, D = data("uniform", N, A, Q)
        k = mixed_k(Q, kmax, seed=N + A, kmin=1)
        run_f64(torch_cuda, X, Qx, D, k, subset(Q, nq, N), kmax,
                f"exact_f64 uniform A={A} N={N} nq={nq} kmax={kmax}",
                expect=None if (A, N) == (1, 2160) else "none")


@pytest.mark.parametrize("A", [5, 8, 16, 32, 64])
def test_exact_f64_near_tie(torch_cuda, A):
    """The screen keeps every near-tied group (P / 4 = 40 groups, 16 per slice at most: below the
    per-slice capacity of either sub-buffer depth, so no query may overflow) and the re-rank
    orders them as the left-to-right sum does."""
    N = RC.N_FILL + NEAR_TIE_P
    X, Qx, D = data("near", N, A, 5)
    for kmax in (16, 32, 64):
        assert NEAR_TIE_P // 4 <= f64_layout(N, A, 4, kmax)["idcap"] - 4
        k = np.array([kmax, kmax, 1, kmax - 3, kmax], np.int32)
        run_f64(torch_cuda, X, Qx, D, k, np.array([4, 0, 2, 1], np.int32), kmax,
                f"exact_f64 near-tie A={A} kmax={kmax}", expect="none")


@pytest.mark.parametrize("kind,expect", [("equal", "all"), ("huge", "all")])
def test_exact_f64_hands_back(torch_cuda, kind, expect):
    """All-equal rows (every group ties with the k-th: more survivors than the refine holds) and
    magnitudes past the fp32 key range: every query reports status 1, its slots [0, k) stay
    untouched and *ovf_count grows by their number."""
    Q = 70
    X, Qx, D = data(kind, 2160, 8, Q)
    k = mixed_k(Q, 16, kmin=1)
    st = run_f64(torch_cuda, X, Qx, D, k, subset(Q, 65), 16, f"exact_f64 {kind}", expect=expect)
    assert (st == 1).all()


# ------------------------------------------------------------------ K4 merge
MERGE_CASES = [
    # L, kin, kout, list_stride - Q * kin      (kernel)
    (1, 8, 12, 4),        # windowed
    (1, 7, 5, 1),         # sequential
    (2, 16, 12, 4),       # windowed, kin > kout
    (2, 16, 20, 1),       # kin % 4 == 0, odd stride: sequential
    (8, 12, 16, 4),       # windowed, kin < kout
    (8, 9, 7, 1),         # sequential
    (9, 8, 12, 4),        # merge path, 4 queries per workgroup
    (9, 250, 256, 1),     # rank kernel (the lists pass 48 KiB of LDS)
    (12, 10, 7, 1),       # merge path
    (12, 16, 100, 4),     # merge path, 1 query per workgroup
    (64, 4, 6, 4),        # merge path
    (64, 44, 40, 1),      # rank kernel, kin > kout
]


@pytest.mark.parametrize("L,kin,kout,pad", MERGE_CASES)
def test_merge_contract(torch_cuda, L, kin, kout, pad):
    """dmlp_merge == merge_ref in every slot of [0, kout) of every row — real entries, then
    (+inf, -1) — for every kernel behind it, with real entries at distance +inf before the
    padding, a list of only such entries merged with lists of only padding, k_q in [0, kout] and
    a list stride larger than Q * kin."""
    torch = torch_cuda
    Q = 130
    lists_d, lists_i, k = RC.merge_lists(L, Q, kin, kout, seed=L * 100 + kin)
    stride = Q * kin + pad
    fd = np.full((L, stride), -5.0)
    fi = np.full((L, stride), -77, np.int32)
    fd[:, :Q * kin] = lists_d.reshape(L, -1)
    fi[:, :Q * kin] = lists_i.reshape(L, -1)
    out = Outputs(torch, Q, kout)
    dd, di, dk = _dev(torch, fd), _dev(torch, fi), _dev(torch, k)
    rc = _lib.lib().dmlp_merge(dd.data_ptr(), di.data_ptr(), L, stride, kin, dk.data_ptr(), Q,
                               out.d.ptr(), out.i.ptr(), kout, _stream(torch))
    assert rc == 0
    ctx = f"merge L={L} kin={kin} kout={kout} stride=Q*kin+{pad}"
    out.d.check_guards(ctx)
    out.i.check_guards(ctx)
    rd, ri = RC.merge_ref(lists_d, lists_i, k, kout)
    np.testing.assert_array_equal(out.i.host(), ri, err_msg=ctx)
    np.testing.assert_array_equal(out.d.host(), rd, err_msg=ctx)
