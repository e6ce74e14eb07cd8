"""Kernel-level contract of the screens and refines, through the C ABI.

The other GPU tests drive the kernels through the dispatcher, which repairs what a kernel gets
wrong (a false overflow or a handed-back query is redone on another path).  These tests call the
screen and refine entry points of dmlp.h directly and check what they WROTE — candidate lists,
counts, thresholds, eps, status — against the float64 reference of tests/helpers/x1_contract.py,
on inputs where the screen's error bound is tight (tests/test_x1_bound_model.py shows that a bound
too small by 2x loses a neighbour of them) and on the generator's uniform data.

Invariants per (query p, slice s) of the single-term screen's lists:
  I1  cand_h[..][1] == eps(q) (rtol 1e-5: a handful of fp32 roundings of the formula)
  I2  cnt >= 0: every oracle neighbour in the slice is a member of a listed group
  I3  cnt >= 0 and the slice has >= k rows: h <= t_s - eps, t_s the k-th largest exact score of
      the slice (slack 2^-22 max(|h|, |t_s|, eps) for the one fp32 subtraction); fewer rows:
      every group with a real row is listed
  I4  0 <= cnt <= 4 (SUB - 2); group indices unique and inside the slice;
      decode(key) <= gmax_exact + eps and decode(key + 1) > gmax_exact - eps
  I5  cnt == -1 only where a slice holds more than 4 (SUB - 2) groups, and never in these cases
"""
import functools
import os
import sys

import numpy as np
import pytest

import distributed_machine_learning_project_amd as dmlp
from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.ops import knn as K

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import result_contract as RC  # noqa: E402
import x1_contract as X1  # noqa: E402

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


def _p(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------ inputs (built once, shared)
# the k of each class: kmax 16 / 32 run the 16-entry screen (56 kept entries: nU + nD = 40 / 56),
# kmax 64 the 32-entry screen (120 kept entries: nU + nD = 104)
K_OF_KMAX = {16: 16, 32: 24, 64: 48}


@functools.lru_cache(maxsize=None)
def adv_case(kind: str, hl: int, A: int, kmax: int, place: str):
    """place: "one" (S = 1), "split" (S = 2, U in slice 0, D in slice 1), "same" (S = 2, both in
    slice 0; twice the rows, so that one slice has a single-member group slot for each)."""
    k = K_OF_KMAX[kmax]
    base = 1024 if kmax == 64 else 512
    N = base * (2 if place == "same" else 1)
    if kind == "subnormal":
        adv = X1.adversarial_subnormal(A, k, N=N)
    else:
        rng = {"one": (None, None), "split": ((N // 2, N), (0, N // 2)),
               "same": ((0, N // 2), (0, N // 2))}[place]
        adv = X1.adversarial_normal(A, k, hl=hl, N=N, d_range=rng[0], u_range=rng[1],
                                    growth=kind == "growth")
    return adv, X1.reference(adv.X, adv.Qx, adv.k, hl=hl)


@functools.lru_cache(maxsize=None)
def uniform_case(A: int, kmax: int, hl: int, N: int = 4096, Q: int = 130, kmin: int = 1):
    inp = dmlp.generate(N, Q, A, 0.0, 1000.0, kmin, kmax, 10, seed=A + kmax)
    return inp, X1.reference(inp.X, inp.Qx, inp.k, hl=hl)


class Ops:
    """The operands of one reference on the device: host-rendered (hl = 1) or written by
    dmlp_prep_data / dmlp_prep_queries (hl = 2, with qlo for the 3-term screens)."""

    def __init__(self, torch, ref, labels, label_range=(0, 10), qidx=None, qk=None):
        """qidx: the query list (distinct rows, any order; None: every row in order), rows on the
        host; qk: a device k array in place of ref.k's (indexed by row, like it)."""
        self.torch, self.ref = torch, ref
        L = self.L = _lib.lib()
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.dev = dev
        self.X, self.Qx = dev(ref.X), dev(ref.Qx)
        self.qk = dev(ref.k.astype(np.int32)) if qk is None else qk
        self.rows = np.arange(ref.Q, dtype=np.int32) if qidx is None \
            else np.ascontiguousarray(qidx, np.int32)
        assert len(np.unique(self.rows)) == len(self.rows) and self.rows.min() >= 0 \
            and self.rows.max() < ref.Q
        self.nq = len(self.rows)
        self.qidx = dev(self.rows)
        self.set_labels(labels, label_range)
        self.words = torch.zeros(2, dtype=torch.int32, device="cuda")  # [0] max norm, [1] bad
        N, A, KT, nt, Q = ref.N, ref.A, ref.KT, ref.n_tiles, ref.Q
        if ref.hl == 1:
            self.xfrag = dev(ref.xhi.view(np.int16))
            self.xinit = dev(ref.xinit)
            self.qhi = dev(ref.qhi.view(np.int16).reshape(-1))
            self.qlo = None
            self.qn = dev(ref.qn)
            self.words[0] = int(ref.xnmax_bits.view(np.int32)[0])
        else:
            mu = dev(ref.mu)
            self.xfrag = torch.zeros(nt * 64 * KT * 32 * 2, dtype=torch.int16, device="cuda")
            self.xinit = torch.zeros(nt * 64, dtype=torch.float32, device="cuda")
            self.qhi = torch.zeros(Q * KT * 32, dtype=torch.int16, device="cuda")
            self.qlo = torch.zeros_like(self.qhi)
            self.qn = torch.zeros(Q, dtype=torch.float32, device="cuda")
            s = _stream(torch)
            w = self.words.data_ptr()
            _lib.check(L.dmlp_prep_data(_p(self.X), N, A, _p(mu), KT, _p(self.xfrag),
                                        _p(self.xinit), w, w + 4, s), "prep_data")
            _lib.check(L.dmlp_prep_queries(_p(self.Qx), Q, A, _p(mu), KT, _p(self.qhi),
                                           _p(self.qlo), _p(self.qn), w + 4, s), "prep_queries")
            torch.cuda.synchronize()
            wh = self.words.cpu().numpy()
            assert wh[1] == 0, "operands outside the screen's range"
            ref.with_norm_word(self.qn.cpu().numpy(), wh[:1])
        self._xrow = None

    def set_labels(self, labels, label_range):
        """the label table and the range [lo, hi) handed to the kernels ((0, 0): not given)"""
        self.labels_h = np.ascontiguousarray(labels, np.int32)
        self.labels = self.dev(self.labels_h)
        self.label_lo, self.label_hi = label_range

    @property
    def xnmax(self):
        return self.words.data_ptr()

    @property
    def bad(self):
        return self.words.data_ptr() + 4

    def xrow(self):
        """the fp16 image point-major (the pair refine's member loads)"""
        if self._xrow is None:
            r = self.ref
            self._xrow = self.torch.zeros(r.n_tiles * 64 * r.KT * 32, dtype=self.torch.int16,
                                          device="cuda")
            _lib.check(self.L.dmlp_x1_rowmajor(_p(self.xfrag), r.n_tiles, r.KT, _p(self._xrow),
                                               _stream(self.torch)), "x1_rowmajor")
        return self._xrow


class Lists:
    """The lists of nq positions and, behind them, a sentinel band of `band` more positions that
    no kernel may write (counts -7, ids -7, h NaN)."""

    def __init__(self, torch, nq, S, cap, band=3):
        self.nq, self.S, self.cap, self.band = nq, S, cap, band
        n = nq + band
        self.ids = torch.zeros(n * S * cap, dtype=torch.int32, device="cuda")
        self.ids[nq * S * cap:] = -7
        self.cnt = torch.full((n * S,), -7, dtype=torch.int32, device="cuda")  # -7: never written
        self.h = torch.full((n * S * 2,), float("nan"), dtype=torch.float32, device="cuda")

    def host(self):
        n = self.nq * self.S
        return (self.ids.cpu().numpy()[:n * self.cap].reshape(self.nq, self.S, self.cap),
                self.cnt.cpu().numpy()[:n].reshape(self.nq, self.S),
                self.h.cpu().numpy()[:2 * n].reshape(self.nq, self.S, 2))

    def check_band(self, ctx=""):
        """the positions past nq still hold their sentinels"""
        n = self.nq * self.S
        assert (self.cnt.cpu().numpy()[n:] == -7).all(), f"{ctx}: a count past nq was written"
        assert (self.ids.cpu().numpy()[n * self.cap:] == -7).all(), f"{ctx}: ids past nq written"
        assert np.isnan(self.h.cpu().numpy()[2 * n:]).all(), f"{ctx}: cand_h past nq written"

    def untouched(self, ctx=""):
        """nothing at all was written: every count -7, every h NaN, the ids as preset"""
        self.check_band(ctx)
        ids, cnt, h = self.host()
        assert (cnt == -7).all() and np.isnan(h).all() and (ids == 0).all(), \
            f"{ctx}: a rejected call wrote into the lists"


NULL = object()   # qk=NULL: a null k pointer (the scalar-k entry points must not read it)


def run_x1(ops, kmax, S, parts=None, qk=None, kuni=None):
    """dmlp_screen_x1, or dmlp_screen_x1_part over the (s_first, S_l) of `parts`; with kuni set,
    dmlp_screen_x1_part_k with that scalar k (over `parts`, or over all S slices at once)."""
    torch, L, r = ops.torch, ops.L, ops.ref
    cap = L.dmlp_screen_x1_cap_kt(r.KT, kmax)
    assert S >= L.dmlp_screen_x1_min_slices(r.n_tiles)
    ls = Lists(torch, ops.nq, S, cap)
    qk = None if qk is NULL else ops.qk if qk is None else qk
    head = (r.KT, r.hl, r.A, _p(ops.xfrag), _p(ops.xinit), r.n_tiles, r.N, _p(ops.qhi),
            _p(ops.qn), _p(ops.qidx), _p(qk))
    mid = (ops.nq, kmax, ops.xnmax, ops.bad, S)
    tail = (_p(ls.ids), _p(ls.cnt), _p(ls.h), _stream(torch))
    if kuni is not None:
        for s_first, S_l in ([(0, S)] if parts is None else parts):
            _lib.check(L.dmlp_screen_x1_part_k(*head, kuni, *mid, s_first, S_l, *tail),
                       "screen_x1_part_k")
    elif parts is None:
        _lib.check(L.dmlp_screen_x1(*head, *mid, *tail), "screen_x1")
    else:
        for s_first, S_l in parts:
            _lib.check(L.dmlp_screen_x1_part(*head, *mid, s_first, S_l, *tail), "screen_x1_part")
    torch.cuda.synchronize()
    ls.check_band("screen_x1")
    return ls


def ready_words(ref, rdy_tiles):
    """Per ready slice of rdy_tiles tiles: the slice's rounded-up max norm as fp32 bits, as the
    host render publishes it (0 is published as 1)."""
    ss = (np.float32(-2.0) * ref.xinit).reshape(ref.n_tiles, 64)
    ss = np.where(np.isfinite(ss), ss, np.float32(0.0)).astype(np.float32)
    up = ss * (np.float32(1.0) + np.float32(1.0e-6)) + np.float32(1.0e-30)
    n = (ref.n_tiles + rdy_tiles - 1) // rdy_tiles
    w = np.zeros(n, np.float32)
    for i in range(n):
        w[i] = up[i * rdy_tiles:(i + 1) * rdy_tiles].max()
    bits = w.view(np.uint32).copy()
    bits[bits == 0] = 1
    return bits


def run_x1_early(ops, kmax, rdy_tiles, qk=None, kuni=None):
    """dmlp_screen_x1_early; with kuni set, dmlp_screen_x1_early_k with that scalar k."""
    torch, L, r = ops.torch, ops.L, ops.ref
    assert r.hl == 1
    cap = L.dmlp_screen_x1_cap_kt(r.KT, kmax)
    ls = Lists(torch, ops.nq, 1, cap)
    qk = None if qk is NULL else ops.qk if qk is None else qk
    bits = ready_words(r, rdy_tiles)
    # the slices' maxima fold to the image's max-norm word: I1 is taken against that
    assert bits.max() == r.xnmax_bits[0]
    rdy = torch.from_numpy(bits.view(np.int32)).cuda()   # preset: nothing can wait
    estats = torch.zeros(3, dtype=torch.int32, device="cuda")
    head = (r.KT, r.A, _p(ops.xfrag), _p(ops.xinit), r.n_tiles, r.N, _p(ops.qhi), _p(ops.qn),
            _p(ops.qidx), _p(qk))
    tail = (ops.nq, kmax, ops.bad, _p(rdy), rdy_tiles, len(bits), _p(ls.ids), _p(ls.cnt),
            _p(ls.h), _p(estats), _stream(torch))
    if kuni is not None:
        _lib.check(L.dmlp_screen_x1_early_k(*head, kuni, *tail), "screen_x1_early_k")
    else:
        _lib.check(L.dmlp_screen_x1_early(*head, *tail), "screen_x1_early")
    torch.cuda.synchronize()
    ls.check_band("screen_x1_early")
    return ls, estats.cpu().numpy()


# ------------------------------------------------------------------ the invariants
def check_lists(ref, ls, grows, k=None, ctx="", thresholds=True, max_ovf_frac=0.0, rows=None):
    """I1 - I5 on the lists of a single-term screen (thresholds=False: a COLLECT pass' lists, whose
    cand_h holds the fixed seed: I1, I2 and the entry checks of I4 only).  rows: the query list —
    list position p is judged against reference row rows[p] (None: position p is row p); k is
    indexed by row, like ref.k."""
    ids, cnt, h = ls.host()
    S, cap = ls.S, ls.cap
    cape = cap - 4 if thresholds else cap     # 4 (SUB - 2) of 4 (SUB - 1); COLLECT: ccap
    k = ref.k if k is None else k
    a_exact, nn_i, eps32 = ref.a_exact, ref.nn_i, ref.eps
    if rows is not None:
        rows = np.asarray(rows, np.int64)
        a_exact, nn_i, eps32, k = a_exact[rows], nn_i[rows], eps32[rows], np.asarray(k)[rows]
    nq = a_exact.shape[0]
    assert cnt.shape == (nq, S), f"{ctx}: lists of {cnt.shape[0]} positions for {nq} queries"
    eps = eps32.astype(np.float64)
    tps = X1.tiles_per_slice(ref.n_tiles, S)
    assert (cnt != -7).all(), f"{ctx}: a (query, slice) count was never written"
    n_ovf = 0
    for s in range(S):
        np.testing.assert_allclose(h[:, s, 1], eps32, rtol=1e-5, err_msg=f"{ctx}: I1 slice {s}")
        r0, r1 = X1.slice_rows(ref.n_tiles, S, s, ref.N)
        nts = max(0, min((s + 1) * tps, ref.n_tiles) - s * tps)
        ae = a_exact[:, r0:r1]
        gmax = X1.group_max(ae, nts, grows)
        ng = gmax.shape[1]
        for p in range(nq):
            where = f"{ctx}: query {p} slice {s}"
            c, kq = int(cnt[p, s]), int(k[p])
            real = np.nonzero(gmax[p] > -np.inf)[0]
            if c < 0:
                assert c == -1, where
                assert len(real) > cape, f"{where}: I5 overflow reported, the buffers cannot fill"
                n_ovf += 1
                continue
            assert 0 <= c <= cape, f"{where}: I4 count {c}"
            e = ids[p, s, :c]
            gi, key = X1.entry_group(e), X1.entry_key(e)
            assert len(np.unique(gi)) == c, f"{where}: I4 duplicate group entries"
            assert (gi < ng).all(), f"{where}: I4 group index outside the slice"
            gm = gmax[p, gi]
            assert (gm > -np.inf).all(), f"{where}: I4 a group of padding rows is listed"
            nn = nn_i[p, :min(kq, ref.N)].astype(np.int64)
            nn = nn[(nn >= r0) & (nn < r1)]
            lost = nn[~np.isin(X1.group_of_row(nn - s * tps * 64, grows), gi)]
            assert len(lost) == 0, f"{where}: I2 oracle neighbours {lost.tolist()} not listed"
            assert (X1.decode16(key) <= gm + eps[p]).all(), f"{where}: I4 key above gmax + eps"
            assert (X1.decode16(key + 1) > gm - eps[p]).all(), f"{where}: I4 key below gmax - eps"
            if not thresholds:
                continue
            if r1 - r0 >= kq >= 1:
                t_s = np.partition(ae[p], -kq)[-kq]
                hs = float(h[p, s, 0])
                slack = 2.0 ** -22 * max(abs(hs), abs(t_s), eps[p])
                assert hs <= t_s - eps[p] + slack, \
                    f"{where}: I3 h {hs!r} above t_s - eps = {t_s - eps[p]!r}"
            elif kq >= 1:
                assert np.isin(real, gi).all(), f"{where}: I3 short slice, a real group is missing"
    assert n_ovf <= max_ovf_frac * nq * S, f"{ctx}: {n_ovf} overflowed (query, slice) pairs"


def grows_of(L, ref, kmax):
    g = L.dmlp_screen_x1_group_rows_kt(ref.KT, kmax)
    # dmlp.h: 8 for the pair epilogue (every 16-entry screen; the 32-entry one at KT 1), else 4
    assert g == (8 if kmax <= 32 or ref.KT == 1 else 4)
    return g


# ------------------------------------------------------------------ refines
class Out:
    def __init__(self, torch, Q, kstride):
        self.kstride = kstride
        self.d = torch.full((Q, kstride), float("nan"), dtype=torch.float64, device="cuda")
        self.i = torch.full((Q, kstride), -9, dtype=torch.int32, device="cuda")
        self.lab = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
        self.cs = torch.full((Q,), -9, dtype=torch.int64, device="cuda")
        self.status = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
        self.ovf = torch.zeros(1, dtype=torch.int32, device="cuda")


def check_refined(ops, out, with_labels, ctx, handed_back=None, rows=None):
    """status == 0 for every query (1 exactly for those of handed_back: a screen overflow), and
    the lists equal the oracle bit for bit (ids, order, distances; label and checksum when voted).
    rows: the query list the refine was given (None: every row in order); handed_back is indexed
    by list position, the outputs by row (the refines write out[q], q = qidx[p]), and the rows of
    unlisted queries keep every sentinel."""
    ops.torch.cuda.synchronize()
    ref = ops.ref
    rows = np.arange(ref.Q) if rows is None else np.asarray(rows, np.int64)
    st = out.status.cpu().numpy()
    want = np.full(ref.Q, -9, np.int32)
    want[rows] = 0 if handed_back is None else np.asarray(handed_back).astype(np.int32)
    assert (st == want).all(), f"{ctx}: status {st.tolist()}"
    assert int(out.ovf.cpu()[0]) == int((want == 1).sum())
    done = np.nonzero(want == 0)[0]
    d, i = out.d.cpu().numpy(), out.i.cpu().numpy()
    un = want == -9
    assert np.isnan(d[un]).all() and (i[un] == -9).all(), f"{ctx}: a row of an unlisted query written"
    assert (out.lab.cpu().numpy()[un] == -9).all() and (out.cs.cpu().numpy()[un] == -9).all(), \
        f"{ctx}: label / checksum of an unlisted query written"
    for q in done:
        kq = min(int(ref.k[q]), ref.N)
        np.testing.assert_array_equal(i[q, :kq], ref.nn_i[q, :kq], err_msg=f"{ctx}: ids q={q}")
        np.testing.assert_array_equal(d[q, :kq], ref.nn_d[q, :kq], err_msg=f"{ctx}: dist q={q}")
    if with_labels:
        lab_ref, cs_ref = K.finalize_cpu(ref.nn_i, ref.k, ops.labels_h)
        lab_py, cs_py = RC.finalize_ref(ref.nn_i, ref.k, ops.labels_h)
        assert (lab_py == lab_ref).all() and (cs_py == cs_ref).all()
        np.testing.assert_array_equal(out.lab.cpu().numpy()[done], lab_ref[done], err_msg=ctx)
        np.testing.assert_array_equal(out.cs.cpu().numpy().view(np.uint64)[done], cs_ref[done],
                                      err_msg=ctx)


def _label_args(ops, out, with_labels):
    return (_p(ops.labels) if with_labels else None, ops.label_lo, ops.label_hi,
            _p(out.lab) if with_labels else None, _p(out.cs) if with_labels else None)


def rows_i32(ops):
    """the lossless int32 rows (x = m / 1e6) of the data and the queries on the device"""
    r = ops.ref
    got = []
    for a in (r.X, r.Qx):
        a = np.ascontiguousarray(a, np.float64)
        m = np.empty(a.shape, np.int32)
        assert ops.L.dmlp_cpu_rows_i32(a.ctypes.data, a.size, m.ctypes.data) == 0, "not 6-decimal"
        got.append(ops.dev(m))
    return got


def refine_rm(ops, ls, kmax, with_labels, ctx, i32=False):
    torch, L, r = ops.torch, ops.L, ops.ref
    pair = L.dmlp_refine_pair_path(ls.S, r.hl, r.KT, int(with_labels), ls.cap, kmax)
    if "DMLP_REFINE_PAIR" not in os.environ:
        assert pair == int(ls.S == 1 and r.hl == 1 and r.KT <= 2 and with_labels and kmax <= 32)
    Xi, Qi = rows_i32(ops) if i32 else (None, None)
    out = Out(torch, r.Q, max(kmax, 1))
    _lib.check(L.dmlp_refine_groups_rm(
        ls.cap, _p(ls.ids), _p(ls.cnt), _p(ls.h), ls.S, _p(ops.X), r.A, _p(ops.Qx), _p(ops.xfrag),
        _p(ops.xrow()) if pair else None, _p(ops.xinit), _p(ops.qhi), r.KT, r.hl, r.N,
        _p(ops.qidx), _p(ops.qk), ops.nq, _p(out.d), _p(out.i), out.kstride,
        *_label_args(ops, out, with_labels), _p(out.status), _p(out.ovf), kmax, _p(Xi), _p(Qi),
        _stream(torch)), "refine_groups_rm")
    check_refined(ops, out, with_labels,
                  f"{ctx} refine_groups_rm pair={pair} labels={with_labels} i32={i32}",
                  rows=ops.rows)
    return pair


def refine_groups(ops, ls, kmax, ctx, collect=None):
    """dmlp_refine_groups (collect None), or dmlp_refine_groups2 with the given collect flag."""
    torch, L, r = ops.torch, ops.L, ops.ref
    out = Out(torch, r.Q, max(kmax, 1))
    args = (ls.cap, _p(ls.ids), _p(ls.cnt), _p(ls.h), ls.S, _p(ops.X), r.A, _p(ops.Qx),
            _p(ops.xfrag), _p(ops.xinit), _p(ops.qhi), r.KT, r.hl, r.N, _p(ops.qidx), _p(ops.qk),
            ops.nq, _p(out.d), _p(out.i), out.kstride, *_label_args(ops, out, True), _p(out.status),
            _p(out.ovf))
    if collect is None:
        _lib.check(L.dmlp_refine_groups(*args, _stream(torch)), "refine_groups")
    else:
        _lib.check(L.dmlp_refine_groups2(*args, collect, _stream(torch)), "refine_groups2")
    check_refined(ops, out, True, f"{ctx} refine_groups collect={collect}", rows=ops.rows)


def screen_and_refine(torch, adv_or_inp, ref, kmax, S, ctx, parts=None, qidx=None):
    ops = Ops(torch, ref, adv_or_inp.labels, qidx=qidx)
    ls = run_x1(ops, kmax, S, parts)
    check_lists(ref, ls, grows_of(ops.L, ref, kmax), ctx=ctx, rows=qidx)
    for with_labels in (True, False):
        refine_rm(ops, ls, kmax, with_labels, ctx)
    refine_groups(ops, ls, kmax, ctx)
    return ops, ls


# ------------------------------------------------------------------ single-term screen: adversarial
@pytest.mark.parametrize("place", ["one", "split", "same"])
@pytest.mark.parametrize("kmax", [16, 32, 64])
@pytest.mark.parametrize("hl,A", [(1, 32), (1, 64), (1, 128), (1, 256), (2, 32), (2, 64)])
def test_x1_adversarial_normal(torch_cuda, hl, A, kmax, place):
    """Coherent rounding in the normal range: the real error is 0.56 eps, family U's scores are too
    high by it and the oracle neighbours' (family D) too low.  KT 2 with kmax <= 32 through
    dmlp_refine_groups failed while dmlp_refine_groups2 took the rows per group from
    group_rows_kt(KT, 64) whatever screen wrote the lists; the bf16 cases (hl = 2) lost family D
    (I2) while the bound took bf16's unit roundoff as 2^-9."""
    adv, ref = adv_case("normal", hl, A, kmax, place)
    S = 1 if place == "one" else 2
    screen_and_refine(torch_cuda, adv, ref, kmax, S, f"normal hl={hl} A={A} kmax={kmax} {place}")


@pytest.mark.parametrize("A", [32, 64])
def test_x1_adversarial_subnormal(torch_cuda, A):
    """fp16 subnormal operands: the rounding error is absolute (half a subnormal step per
    attribute) and only the bound's r3 term covers it."""
    adv, ref = adv_case("subnormal", 1, A, 16, "one")
    screen_and_refine(torch_cuda, adv, ref, 16, 1, f"subnormal A={A}")


# ------------------------------------------------------------------ single-term screen: uniform data
@pytest.mark.parametrize("A,kmax", [(32, 16), (40, 32)])
def test_x1_uniform(torch_cuda, A, kmax):
    """The generator's distribution: no (query, slice) overflows, S = 1 and S = 4, and
    dmlp_screen_x1_part over slices [0, 2) and [2, 4) writes the single launch's lists."""
    inp, ref = uniform_case(A, kmax, 1)
    ctx = f"uniform A={A} kmax={kmax}"
    screen_and_refine(torch_cuda, inp, ref, kmax, 1, ctx + " S=1")
    ops, whole = screen_and_refine(torch_cuda, inp, ref, kmax, 4, ctx + " S=4")
    part = run_x1(ops, kmax, 4, parts=[(0, 2), (2, 2)])
    check_lists(ref, part, grows_of(ops.L, ref, kmax), ctx=ctx + " parts")
    (i0, c0, h0), (i1, c1, h1) = whole.host(), part.host()
    np.testing.assert_array_equal(c1, c0)
    np.testing.assert_array_equal(h1, h0)
    live = np.arange(whole.cap).reshape(1, 1, -1) < c0[:, :, None]
    np.testing.assert_array_equal(np.where(live, i1, 0), np.where(live, i0, 0))


# ------------------------------------------------------------------ early start
@pytest.mark.parametrize("kind,A", [("normal", 32), ("normal", 64), ("growth", 32), ("growth", 128)])
def test_x1_early_preset(torch_cuda, kind, A):
    """dmlp_screen_x1_early with every ready word preset to its slice's max norm: nothing waits,
    eps is the final one (I1 against the whole image's max norm), I2 - I4 as for the plain screen,
    and the refine of its lists equals the oracle."""
    adv, ref = adv_case(kind, 1, A, 16, "one")
    ops = Ops(torch_cuda, ref, adv.labels)
    ls, estats = run_x1_early(ops, 16, rdy_tiles=2)
    assert estats[2] == 0, "an early-start wave timed out on preset ready words"
    ctx = f"early {kind} A={A}"
    check_lists(ref, ls, grows_of(ops.L, ref, 16), ctx=ctx)
    refine_rm(ops, ls, 16, True, ctx)
    refine_groups(ops, ls, 16, ctx)


# ------------------------------------------------------------------ two-pass large k
def run_x1_collect(ops, hseed, ccap, S):
    """dmlp_screen_x1_collect at the seeds hseed (per list position)"""
    torch, L, r = ops.torch, ops.L, ops.ref
    ls = Lists(torch, ops.nq, S, ccap)
    _lib.check(L.dmlp_screen_x1_collect(
        r.KT, r.A, _p(ops.xfrag), _p(ops.xinit), r.n_tiles, r.N, _p(ops.qhi), _p(ops.qn),
        _p(ops.qidx), _p(ops.qk), ops.nq, ops.xnmax, ops.bad, _p(hseed), ccap, S, _p(ls.ids),
        _p(ls.cnt), _p(ls.h), _stream(torch)), "screen_x1_collect")
    torch.cuda.synchronize()
    ls.check_band("screen_x1_collect")
    return ls


def first_pass_seed(ops, S1):
    """The two-pass form's first pass: k' = ceil(k / S1) per row over S1 slices, then dmlp_x1_seed
    -> (the first pass' lists, k' by row, the seeds by list position)."""
    torch, r = ops.torch, ops.ref
    kp = ((np.maximum(r.k, 1) + S1 - 1) // S1).astype(np.int32)
    first = run_x1(ops, int(kp.max()), S1, qk=torch.from_numpy(kp).cuda())
    hseed = torch.full((ops.nq,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(ops.L.dmlp_x1_seed(_p(first.h), _p(first.cnt), S1, ops.nq, _p(hseed),
                                  _stream(torch)), "x1_seed")
    return first, kp, hseed


@pytest.mark.parametrize("k", [33, 100, 256])
@pytest.mark.parametrize("A", [32, 100])
def test_x1_two_pass(torch_cuda, A, k):
    """k' = ceil(k / 16) over S1 = 16 slices -> dmlp_x1_seed -> dmlp_screen_x1_collect: the seed
    is at most t - eps (t: the k-th best exact score over all points), the COLLECT lists hold every
    oracle neighbour (4-row groups), a +inf seed reports overflow in every slice, and
    dmlp_refine_groups2(collect = 1) on the lists equals the oracle."""
    torch = torch_cuda
    inp, ref = uniform_case(A, k, 1, N=2048, Q=70, kmin=k)
    ops = Ops(torch, ref, inp.labels)
    L, S1, S2, ccap = ops.L, 16, 2, 1024
    kp = ((np.maximum(ref.k, 1) + S1 - 1) // S1).astype(np.int32)
    kmax1 = int(kp.max())
    first = run_x1(ops, kmax1, S1, qk=torch.from_numpy(kp).cuda())
    ctx = f"two-pass A={A} k={k}"
    check_lists(ref, first, grows_of(L, ref, kmax1), k=kp, ctx=ctx + " first pass")
    hseed = torch.full((ref.Q,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(L.dmlp_x1_seed(_p(first.h), _p(first.cnt), S1, ref.Q, _p(hseed), _stream(torch)),
               "x1_seed")

    def collect(seed):
        return run_x1_collect(ops, seed, ccap, S2)

    ls = collect(hseed)
    hs = hseed.cpu().numpy().astype(np.float64)
    eps = ref.eps.astype(np.float64)
    for p in range(ref.Q):
        t = np.partition(ref.a_exact[p], -k)[-k]
        slack = 2.0 ** -22 * max(abs(hs[p]), abs(t), eps[p])
        assert hs[p] <= t - eps[p] + slack, f"{ctx}: seed of query {p} above t - eps"
    check_lists(ref, ls, 4, ctx=ctx + " collect", thresholds=False)
    refine_groups(ops, ls, k, ctx, collect=1)
    # a +inf seed (a first-pass slice overflowed): every slice of that query reports -1
    dead = [0, 65]
    seed2 = hseed.clone()
    seed2[dead] = float("inf")
    c2 = collect(seed2).host()[1]
    assert (c2[dead] == -1).all()
    alive = np.setdiff1d(np.arange(ref.Q), dead)
    np.testing.assert_array_equal(c2[alive], ls.host()[1][alive])


# ------------------------------------------------------------------ 3-term screens: completeness
def check_id_lists(ref, ids, cnt, S, ctx, rows=None):
    """Every oracle neighbour of a slice is in the slice's candidate list (global point ids, as
    dmlp_refine reads them), or the count is -1.  rows: the query list (position p is row rows[p];
    None: row p)."""
    tps = X1.tiles_per_slice(ref.n_tiles, S)
    rows = np.arange(ref.Q) if rows is None else np.asarray(rows, np.int64)
    assert cnt.shape == (len(rows), S)
    for s in range(S):
        r0, r1 = X1.slice_rows(ref.n_tiles, S, s, ref.N)
        for p, q in enumerate(rows):
            c = int(cnt[p, s])
            if c < 0:
                assert c == -1
                continue
            assert c <= ids.shape[2], f"{ctx}: query {p} slice {s}: count past the list"
            nn = ref.nn_i[q, :min(int(ref.k[q]), ref.N)]
            nn = nn[(nn >= r0) & (nn < r1)]
            lost = nn[~np.isin(nn, ids[p, s, :c])]
            assert len(lost) == 0, f"{ctx}: query {p} slice {s}: neighbours {lost.tolist()} not listed"


def three_term(torch, src, ref, impl, cap, kmax, S, ctx, max_ovf_frac=0.05, qidx=None):
    """A 3-term screen and dmlp_refine on its lists: every list is complete or reports overflow
    (at most max_ovf_frac of the (query, slice) pairs); the refine hands back exactly the
    overflowed queries (status 1) and equals the oracle on every other."""
    ops = Ops(torch, ref, src.labels, qidx=qidx)
    L = ops.L
    er = np.float32(K.eps_rel(ref.A))
    ls = Lists(torch, ops.nq, S, cap)     # (cand_h is not used: its NaNs must stay)
    ids, cnt = ls.ids, ls.cnt
    head = (_p(ops.xfrag), _p(ops.xinit), ref.n_tiles, _p(ops.qhi), _p(ops.qlo), _p(ops.qn),
            _p(ops.qidx), _p(ops.qk), ops.nq)
    tail = (ops.xnmax, ops.bad, er, S, _p(ids), _p(cnt), _stream(torch))
    if impl == "stream":
        assert cap == L.dmlp_screen_stream_cap(kmax) and L.dmlp_screen_stream_qw(ref.KT) > 0
        _lib.check(L.dmlp_screen_stream(ref.KT, *head, kmax, *tail), "screen_stream")
    else:
        assert kmax <= L.dmlp_screen_kmax(cap) and L.dmlp_screen_waves_hl(ref.KT, cap, 2) > 0
        _lib.check(L.dmlp_screen(ref.KT, cap, *head, *tail), "screen")
    torch.cuda.synchronize()
    ls.check_band(ctx)
    ids_h, cnt_h, h_h = ls.host()
    assert np.isnan(h_h).all()
    assert (cnt_h != -7).all()
    check_id_lists(ref, ids_h, cnt_h, S, ctx, rows=qidx)
    ovf = (cnt_h < 0).any(axis=1)
    assert (cnt_h < 0).sum() <= max_ovf_frac * cnt_h.size, \
        f"{ctx}: {(cnt_h < 0).sum()} of {cnt_h.size} (query, slice) pairs overflowed"
    out = Out(torch, ref.Q, kmax)
    _lib.check(L.dmlp_refine(cap, _p(ids), _p(cnt), S, _p(ops.X), ref.A, _p(ops.Qx), _p(ops.qidx),
                             _p(ops.qk), ops.nq, _p(out.d), _p(out.i), out.kstride,
                             *_label_args(ops, out, True), _p(out.status), _p(out.ovf),
                             _stream(torch)), "refine")
    check_refined(ops, out, True, ctx + " refine", handed_back=ovf, rows=qidx)


@pytest.mark.parametrize("data", ["uniform", "adversarial", "adversarial16"])
@pytest.mark.parametrize("A", [32, 64])
def test_screen_stream_complete(torch_cuda, data, A):
    """adversarial: k = 16 in the class kmax = 32 (16-entry buffers).  adversarial16: the same
    queries in the class kmax = 16, whose 8-entry buffers cannot hold the 40 tied groups of the two
    families: overflow is the contract's answer there, and the refine must hand those queries
    back."""
    L = _lib.lib()
    if data == "uniform":
        kmax, frac = 32, 0.05
        src, ref = uniform_case(A, kmax, 2)
    else:
        kmax, frac = (32, 0.05) if data == "adversarial" else (16, 1.0)
        src, ref = adv_case("normal", 2, A, 16, "one")
    for S in (1, 3):
        three_term(torch_cuda, src, ref, "stream", L.dmlp_screen_stream_cap(kmax), kmax, S,
                   f"stream {data} A={A} S={S}", max_ovf_frac=frac)


@pytest.mark.parametrize("cap,kmax", [(128, 32), (256, 128), (512, 256)])
@pytest.mark.parametrize("data,A", [("uniform", 32), ("uniform", 40), ("adversarial", 64)])
def test_screen_lds_complete(torch_cuda, data, A, cap, kmax):
    if data == "uniform":
        src, ref = uniform_case(A, kmax, 2)
    else:
        src, ref = adv_case("normal", 2, A, 16, "one")
        kmax = 16
    for S in (1, 3):
        three_term(torch_cuda, src, ref, "lds", cap, kmax, S,
                   f"lds {data} A={A} cap={cap} S={S}")


# ------------------------------------------------------------------ votes through every fused kernel
# Every label space of tests/helpers/result_contract.py through every entry point that takes
# labels.  dmlp::wave_vote_by takes its LDS histogram when 0 < hi - lo <= hist_cap (512 in
# k_finalize and the candidate-list k_refine, 256 in the group forms of k_refine) and counts
# otherwise; k_refine votes on labels carried in LDS or through finalize_wave; k_refine_pair has a
# count loop of its own.  Expected: vote_ref / fnv_ref on the oracle's neighbour lists, bit for
# bit ("two" and "distinct" break a wrong tie rule, "r256" .. "r513" sit on both sides of both
# caps, "extreme" / "extreme_lo" have ranges no int holds).
VOTE_SPACES = list(RC.LABEL_SPACES)
_VOTE_SETUPS = {}


def lds_lists(ops, cap, kmax, S):
    """the 3-term LDS screen's candidate id lists (dmlp_refine's input)"""
    torch, L, ref = ops.torch, ops.L, ops.ref
    assert kmax <= L.dmlp_screen_kmax(cap) and L.dmlp_screen_waves_hl(ref.KT, cap, 2) > 0
    ids = torch.zeros(ref.Q * S * cap, dtype=torch.int32, device="cuda")
    cnt = torch.full((ref.Q * S,), -7, dtype=torch.int32, device="cuda")
    _lib.check(L.dmlp_screen(ref.KT, cap, _p(ops.xfrag), _p(ops.xinit), ref.n_tiles, _p(ops.qhi),
                             _p(ops.qlo), _p(ops.qn), _p(ops.qidx), _p(ops.qk), ref.Q, ops.xnmax,
                             ops.bad, np.float32(K.eps_rel(ref.A)), S, _p(ids), _p(cnt),
                             _stream(torch)), "screen")
    torch.cuda.synchronize()
    ovf = (cnt.cpu().numpy().reshape(ref.Q, S) < 0).any(axis=1)
    assert ovf.mean() <= 0.05
    return ids, cnt, ovf


def collect_lists(ops, k):
    """the two-pass large-k lists (dmlp_refine_groups2 collect = 1), as test_x1_two_pass"""
    S1, S2, ccap = 16, 2, 1024
    _, _, hseed = first_pass_seed(ops, S1)
    return run_x1_collect(ops, hseed, ccap, S2)


def vote_setup(torch, name):
    """One uniform input per kernel class (N = 4096, Q = 130 in two ragged query blocks, k mixed
    in [1, kmax]; the two-pass class N = 2048, Q = 70, k = 100), screened once and shared."""
    if name not in _VOTE_SETUPS:
        A, kmax, hl, kw = {"a32": (32, 16, 1, {}), "a40": (40, 32, 1, {}), "k64": (32, 64, 1, {}),
                           "collect": (100, 100, 1, dict(N=2048, Q=70, kmin=100)),
                           "lds128": (32, 32, 2, {}), "lds256": (32, 128, 2, {})}[name]
        inp, ref = uniform_case(A, kmax, hl, **kw)
        ops = Ops(torch, ref, inp.labels)
        if name.startswith("lds"):
            lists = lds_lists(ops, int(name[3:]), kmax, 1)
        elif name == "collect":
            lists = collect_lists(ops, kmax)
        else:
            lists = {S: run_x1(ops, kmax, S) for S in ((1,) if name == "k64" else (1, 4))}
        _VOTE_SETUPS[name] = (ops, lists, kmax)
    return _VOTE_SETUPS[name]


def with_space(torch, name, space):
    ops, lists, kmax = vote_setup(torch, name)
    labels, lo, hi = RC.label_space(space, ops.ref.N)
    ops.set_labels(labels, (lo, hi))
    return ops, lists, kmax


@pytest.mark.parametrize("cap", [128, 256])
@pytest.mark.parametrize("space", VOTE_SPACES)
def test_votes_refine(torch_cuda, space, cap):
    """dmlp_refine (k_refine<4, 0>, hist_cap 512) on the LDS screen's lists, cap 128 and 256."""
    ops, (ids, cnt, ovf), kmax = with_space(torch_cuda, f"lds{cap}", space)
    torch, ref = ops.torch, ops.ref
    out = Out(torch, ref.Q, kmax)
    _lib.check(ops.L.dmlp_refine(cap, _p(ids), _p(cnt), 1, _p(ops.X), ref.A, _p(ops.Qx),
                                 _p(ops.qidx), _p(ops.qk), ref.Q, _p(out.d), _p(out.i), out.kstride,
                                 *_label_args(ops, out, True), _p(out.status), _p(out.ovf),
                                 _stream(torch)), "refine")
    check_refined(ops, out, True, f"votes {space} refine cap={cap}", handed_back=ovf)


@pytest.mark.parametrize("setup,S", [("a32", 1), ("a32", 4), ("a40", 1), ("a40", 4), ("k64", 1)])
@pytest.mark.parametrize("space", VOTE_SPACES)
def test_votes_refine_groups(torch_cuda, space, setup, S):
    """dmlp_refine_groups and dmlp_refine_groups2(collect = 0): the group forms of k_refine
    (hist_cap 256, labels carried in LDS), KT 1 and 2, one slice and four."""
    ops, lists, kmax = with_space(torch_cuda, setup, space)
    ctx = f"votes {space} {setup} S={S}"
    refine_groups(ops, lists[S], kmax, ctx)
    refine_groups(ops, lists[S], kmax, ctx, collect=0)


@pytest.mark.parametrize("space", VOTE_SPACES)
def test_votes_refine_groups_collect(torch_cuda, space):
    """dmlp_refine_groups2(collect = 1): k = 100 at A = 100 (k_refine<8, 4, true>, which votes
    through finalize_wave)."""
    ops, ls, kmax = with_space(torch_cuda, "collect", space)
    refine_groups(ops, ls, kmax, f"votes {space} collect", collect=1)


@pytest.mark.parametrize("setup,S,i32", [("a32", 1, False), ("a32", 1, True), ("a40", 1, False),
                                         ("a40", 1, True), ("a32", 4, False), ("a40", 4, False),
                                         ("k64", 1, False), ("a32", 4, True), ("a40", 4, True),
                                         ("k64", 1, True)])
@pytest.mark.parametrize("space", VOTE_SPACES)
def test_votes_refine_groups_rm(torch_cuda, space, setup, S, i32):
    """dmlp_refine_groups_rm on the pair path (S = 1, k <= 32: k_refine_pair's own count loop)
    and off it (S = 4, or the class k <= 64: k_refine), each with fp64 rows and with the lossless
    int32 rows Xi / Qi (off the pair path k_refine reads Xi for the data and Qx for the query)."""
    ops, lists, kmax = with_space(torch_cuda, setup, space)
    pair = refine_rm(ops, lists[S], kmax, True, f"votes {space} {setup} S={S}", i32=i32)
    if "DMLP_REFINE_PAIR" not in os.environ:
        assert pair == int(S == 1 and kmax <= 32)


@functools.lru_cache(maxsize=None)
def finalize_lists():
    """Q = 130 rows of distinct ids of N = 200 points with stride 300, k in {0, 1, 2, 16, 64, 256,
    300}: k > N rows end in padding, which the vote skips and the checksum covers."""
    rng = np.random.default_rng(9)
    N, Q, ks = 200, 130, 300
    k = np.array([0, 1, 2, 16, 64, 256, 300], np.int32)[rng.integers(0, 7, Q)]
    k[:7] = [0, 1, 2, 16, 64, 256, 300]
    ids = np.full((Q, ks), -1, np.int32)
    for q in range(Q):
        ids[q, :N] = rng.permutation(N)
    ids[7, :] = -1                  # a row of padding only, k = 300
    k[7] = 300
    return N, ids, k


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("space", VOTE_SPACES)
def test_votes_finalize(torch_cuda, space, listed):
    """dmlp_finalize (hist_cap 512) on all rows and on an unsorted subset of them (qidx); rows
    that are not listed keep their label and checksum words."""
    torch = torch_cuda
    N, ids, k = finalize_lists()
    Q, ks = ids.shape
    labels, lo, hi = RC.label_space(space, N)
    qidx = np.random.default_rng(4).permutation(Q)[:77].astype(np.int32) if listed else None
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lab = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
    cs = torch.full((Q,), -9, dtype=torch.int64, device="cuda")
    d_ids, d_k, d_lab, d_q = dev(ids), dev(k), dev(labels), (dev(qidx) if listed else None)
    _lib.check(_lib.lib().dmlp_finalize(None, _p(d_ids), ks, _p(d_k), _p(d_q),
                                        len(qidx) if listed else Q, _p(d_lab), lo, hi, _p(lab),
                                        _p(cs), _stream(torch)), "finalize")
    torch.cuda.synchronize()
    lab_ref, cs_ref = RC.finalize_ref(ids, k, labels)
    rows = np.zeros(Q, bool)
    rows[qidx if listed else slice(None)] = True
    got_lab, got_cs = lab.cpu().numpy(), cs.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got_lab[rows], lab_ref[rows])
    np.testing.assert_array_equal(got_cs[rows], cs_ref[rows])
    assert (got_lab[~rows] == -9).all() and (got_cs[~rows].view(np.int64) == -9).all()


@functools.lru_cache(maxsize=None)
def dispatch_case(A: int):
    """The uniform input of the vote setups with k over every class of the dispatcher: 0, the
    single-term classes, the LDS screen's, the exact paths', and k > N (padding in the checksum)."""
    inp, _ = uniform_case(A, {32: 16, 40: 32}[A], 1)
    N, Q = inp.X.shape[0], inp.Qx.shape[0]
    rng = np.random.default_rng(A)
    k = rng.integers(1, 65, Q).astype(np.int32)
    k[:12] = [0, 1, 16, 17, 32, 33, 64, 65, 256, 300, N, N + 5]
    k[Q - 1] = 0
    ks = N + 5
    d, i = RC.knn_ref(inp.X, inp.Qx, k, ks)
    return inp, k, ks, d, i


def check_dispatch(inp, k, d_ref, i_ref, labels, got, ctx):
    d, i, lab, cs = (t.cpu().numpy() for t in got)
    for q in range(len(k)):
        np.testing.assert_array_equal(i[q, :k[q]], i_ref[q, :k[q]], err_msg=f"{ctx}: ids q={q}")
        np.testing.assert_array_equal(d[q, :k[q]], d_ref[q, :k[q]], err_msg=f"{ctx}: dist q={q}")
    lab_ref, cs_ref = RC.finalize_ref(i_ref, k, labels)
    np.testing.assert_array_equal(lab, lab_ref, err_msg=ctx)
    np.testing.assert_array_equal(cs.view(np.uint64), cs_ref, err_msg=ctx)


@pytest.mark.parametrize("A", [32, 40])
@pytest.mark.parametrize("space", VOTE_SPACES)
def test_votes_knn_local(torch_cuda, space, A):
    """dmlp_knn_local: every refine of the dispatcher and finalize_rest behind one call."""
    torch = torch_cuda
    inp, k, ks, d_ref, i_ref = dispatch_case(A)
    labels, lo, hi = RC.label_space(space, inp.X.shape[0])
    ds = K.prepare_dataset(torch.from_numpy(inp.X).cuda(), torch.from_numpy(labels).cuda(), (lo, hi))
    r = K.knn_gpu(ds, torch.from_numpy(inp.Qx).cuda(), k, kstride=ks)
    torch.cuda.synchronize()
    check_dispatch(inp, k, d_ref, i_ref, labels, (r.dist, r.ids, r.label, r.checksum),
                   f"votes {space} knn_local A={A}")


@pytest.mark.parametrize("A", [32, 40])
@pytest.mark.parametrize("space", VOTE_SPACES)
def test_votes_step(torch_cuda, space, A):
    """dmlp_step from host rows, k = 0 and k > N included.  A range of (0, 0) is scanned by the
    step itself: for "extreme" the scan meets INT_MAX, whose exclusive bound no int holds."""
    torch = torch_cuda
    inp, k, ks, d_ref, i_ref = dispatch_case(A)
    labels, lo, hi = RC.label_space(space, inp.X.shape[0])
    r = K.step(inp.X, labels, (lo, hi), inp.Qx, k, lists=True, kstride=ks)
    torch.cuda.synchronize()
    check_dispatch(inp, k, d_ref, i_ref, labels, (r.dist, r.ids, r.label, r.checksum),
                   f"votes {space} step A={A}")


# ------------------------------------------------------------------ padding and handed-back rows
class GuardedOut:
    """Out with sentinel bands around the lists (tests/helpers/result_contract.py: guarded)."""

    def __init__(self, torch, Q, kstride):
        self.kstride = kstride
        self.gd = RC.guarded(torch, (Q, kstride), torch.float64)
        self.gi = RC.guarded(torch, (Q, kstride), torch.int32)
        self.d, self.i = self.gd.t, self.gi.t
        self.lab = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
        self.cs = torch.zeros(Q, dtype=torch.int64, device="cuda")
        self.status = torch.full((Q,), -9, dtype=torch.int32, device="cuda")
        self.ovf = torch.zeros(1, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("entry", ["refine", "groups", "groups_rm", "pair"])
def test_refine_pads_every_listed_row(torch_cuda, entry):
    """dmlp.h: with kstride > kmax every refine writes (+inf, -1) into [k_q, kstride) of every
    listed row, handed-back ones included; a handed-back row (a slice count of -1) keeps its slots
    [0, k_q) untouched and reports status 1; nothing outside the lists is written."""
    torch = torch_cuda
    setup = {"refine": "lds128", "groups": "a32", "groups_rm": "a32", "pair": "a32"}[entry]
    ops, lists, kmax = with_space(torch, setup, "ten")
    ref, L = ops.ref, ops.L
    back = np.zeros(ref.Q, bool)
    back[[0, 65, ref.Q - 1]] = True
    out = GuardedOut(torch, ref.Q, kmax + 5)
    tail = (_p(ops.qidx), _p(ops.qk), ref.Q, _p(out.d), _p(out.i), out.kstride,
            *_label_args(ops, out, True), _p(out.status), _p(out.ovf))
    if entry == "refine":
        ids, cnt, ovf = lists
        cnt = cnt.clone()
        cnt[torch.from_numpy(np.nonzero(back)[0]).cuda()] = -1
        back |= ovf
        _lib.check(L.dmlp_refine(128, _p(ids), _p(cnt), 1, _p(ops.X), ref.A, _p(ops.Qx), *tail,
                                 _stream(torch)), "refine")
    else:
        S = 1 if entry == "pair" else 4
        ls = lists[S]
        cnt = ls.cnt.clone()
        cnt[torch.from_numpy(np.nonzero(back)[0] * S + S - 1).cuda()] = -1   # the last slice's
        head = (ls.cap, _p(ls.ids), _p(cnt), _p(ls.h), S, _p(ops.X), ref.A, _p(ops.Qx),
                _p(ops.xfrag))
        mid = (_p(ops.xinit), _p(ops.qhi), ref.KT, ref.hl, ref.N)
        if entry == "groups":
            _lib.check(L.dmlp_refine_groups(*head, *mid, *tail, _stream(torch)), "refine_groups")
        else:
            pair = L.dmlp_refine_pair_path(S, ref.hl, ref.KT, 1, ls.cap, kmax)
            if "DMLP_REFINE_PAIR" not in os.environ:
                assert pair == int(entry == "pair")
            _lib.check(L.dmlp_refine_groups_rm(*head, _p(ops.xrow()) if pair else None, *mid,
                                               *tail, kmax, None, None, _stream(torch)),
                       "refine_groups_rm")
    ctx = f"padding {entry}"
    out.gd.check_guards(ctx)
    out.gi.check_guards(ctx)
    d, i = out.gd.host(), out.gi.host()
    np.testing.assert_array_equal(out.status.cpu().numpy(), back.astype(np.int32), err_msg=ctx)
    assert int(out.ovf.cpu()[0]) == int(back.sum())
    keep = np.zeros(d.shape, bool)
    for q in range(ref.Q):
        kq = int(ref.k[q])
        assert (i[q, kq:] == -1).all() and np.isposinf(d[q, kq:]).all(), \
            f"{ctx}: row {q} slots [{kq}, {out.kstride}) are not (+inf, -1)"
        if back[q]:
            keep[q, :kq] = True
        else:
            np.testing.assert_array_equal(i[q, :kq], ref.nn_i[q, :kq], err_msg=f"{ctx}: ids {q}")
            np.testing.assert_array_equal(d[q, :kq], ref.nn_d[q, :kq], err_msg=f"{ctx}: dist {q}")
    out.gd.untouched(keep, ctx)
    out.gi.untouched(keep, ctx)
