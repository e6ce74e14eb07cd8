"""The screens under the launch geometry production uses, through the C ABI.

tests/test_screen_contract.py, test_screen_x1_schedule.py and test_screen_check_cadence.py run every
screen with qidx = arange(Q), S <= 5, k from the qk array, KT <= 2 on the bf16 image and slices of
at most 64 tiles.  The dispatcher (Local::pass in csrc/local.h) runs them differently, and this file
runs them that way:

  A  query subsets   an unsorted class subset (77 of 130 rows; 41 of 70 for the two-pass form):
                     the kernels index the lists, hseed and cand_h by list position p, the
                     operands, qn and qk by row q = qidx[p], the refines' outputs by row again
  B  block map       S = 8 and 16 (the XCD-aware decode of blockIdx.x, with 3 query blocks), ragged
                     and empty slices, dmlp_screen_x1_part launches whose S_l picks one decode while
                     S lays out the lists
  C  scalar k        dmlp_screen_x1_part_k / dmlp_screen_x1_early_k with kuni >= 0 and a null or
                     poisoned qk
  D  instantiations  the bf16 image at KT 4 and 8, the early form at KT 8 and with 32-entry
                     buffers, the COLLECT pass at KT 2 and 8
  E  full slice      one slice of 4096 tiles: group indices up to 32767 (8-row groups) and 65535
                     (4-row groups), and the rejection of 4097 tiles
  F  argument errors of dmlp_screen_x1_part, which must write nothing

Every list is judged by invariants I1 - I5 of test_screen_contract.py (check_lists / check_id_lists
with rows = the query list), every list array ends in a sentinel band that must survive, and every
refine result equals the float64 oracle bit for bit, with the rows of unlisted queries untouched.
The cases and their data come from tests/test_screen_geometry_model.py, which shows on the CPU that
the checker accepts the reference's ideal lists for them, that those lists cannot overflow, and that
it rejects what each bug aimed at here would write.  Every ready word of an early-start case is
preset: no wave waits.
"""
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
for _d in (HERE, os.path.join(HERE, "helpers")):
    if _d not in sys.path:
        sys.path.insert(0, _d)
import test_screen_contract as TSC  # noqa: E402  (Ops, the runners, check_lists: I1 - I5)
import test_screen_geometry_model as GM  # noqa: E402  (the cases and their data)
import x1_contract as X1  # noqa: E402

pytestmark = pytest.mark.gpu
QLIST, QLIST41 = GM.QLIST, GM.QLIST41
_p, _stream = TSC._p, TSC._stream


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch


def same_lists(a, b, ctx):
    """per (p, s): counts equal, entries equal as sets, cand_h equal on its bits"""
    (i0, c0, h0), (i1, c1, h1) = a.host(), b.host()
    np.testing.assert_array_equal(c1, c0, err_msg=f"{ctx}: counts")
    np.testing.assert_array_equal(h1.view(np.uint32), h0.view(np.uint32), err_msg=f"{ctx}: cand_h")
    live = np.arange(a.cap).reshape(1, 1, -1) < c0[:, :, None]
    big = np.iinfo(np.int32).max
    np.testing.assert_array_equal(np.sort(np.where(live, i1, big), axis=2),
                                  np.sort(np.where(live, i0, big), axis=2),
                                  err_msg=f"{ctx}: entries")


def no_overflow(ls, ctx):
    cnt = ls.host()[1]
    assert (cnt >= 0).all(), f"{ctx}: counts {np.unique(cnt).tolist()}"


def x1_and_check(torch, case):
    """dmlp_screen_x1 on one case of the model file; I1 - I5 with its query list"""
    name, dat, S, rows = case
    inp, ref = GM.data(*dat)
    kmax = dat[2]
    ops = TSC.Ops(torch, ref, inp.labels, qidx=rows)
    ls = TSC.run_x1(ops, kmax, S)
    TSC.check_lists(ref, ls, TSC.grows_of(ops.L, ref, kmax), ctx=name, rows=rows)
    no_overflow(ls, name)
    return ops, ls


# ================================================================== A. query subsets
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("hl,A,kmax", GM.SUBSET_SHAPES)
def test_subset_x1(torch_cuda, hl, A, kmax, S):
    """dmlp_screen_x1 on the 77-row list, then dmlp_refine_groups_rm (on the pair path at hl 1,
    A 32, kmax 16, S 1 with labels; off it everywhere else) and dmlp_refine_groups."""
    inp, ref = GM.data(GM.kind_of(hl, kmax), A, kmax, hl)
    ctx = f"subset hl={hl} A={A} kmax={kmax} S={S}"
    _, ls = TSC.screen_and_refine(torch_cuda, inp, ref, kmax, S, ctx, qidx=QLIST)
    no_overflow(ls, ctx)


def test_subset_x1_early(torch_cuda):
    inp, ref = GM.data("base", 32, 16, 1)
    ops = TSC.Ops(torch_cuda, ref, inp.labels, qidx=QLIST)
    ls, estats = TSC.run_x1_early(ops, 16, rdy_tiles=2)
    assert estats[0] == 0 and estats[2] == 0, f"waits {estats[0]}, timeouts {estats[2]}"
    ctx = "subset early"
    TSC.check_lists(ref, ls, TSC.grows_of(ops.L, ref, 16), ctx=ctx, rows=QLIST)
    same_lists(TSC.run_x1(ops, 16, 1), ls, ctx + " against the plain screen")
    assert TSC.refine_rm(ops, ls, 16, True, ctx) == 1 or "DMLP_REFINE_PAIR" in os.environ
    TSC.refine_groups(ops, ls, 16, ctx)


def two_pass(torch, A, rows, ctx):
    """first pass -> dmlp_x1_seed -> dmlp_screen_x1_collect -> dmlp_refine_groups2(collect = 1) on
    the k = 100 case of test_x1_two_pass (N = 2048, Q = 70)"""
    k, S1, S2, ccap = 100, 16, 2, 1024
    inp, ref = TSC.uniform_case(A, k, 1, N=2048, Q=70, kmin=k)
    ops = TSC.Ops(torch, ref, inp.labels, qidx=rows)
    first, kp, hseed = TSC.first_pass_seed(ops, S1)
    TSC.check_lists(ref, first, TSC.grows_of(ops.L, ref, int(kp.max())), k=kp,
                    ctx=ctx + " first pass", rows=rows)
    hs = hseed.cpu().numpy().astype(np.float64)
    eps = ref.eps.astype(np.float64)
    for p, q in enumerate(ops.rows):
        t = np.partition(ref.a_exact[q], -k)[-k]
        slack = 2.0 ** -22 * max(abs(hs[p]), abs(t), eps[q])
        assert hs[p] <= t - eps[q] + slack, f"{ctx}: seed of position {p} above t - eps"
    ls = TSC.run_x1_collect(ops, hseed, ccap, S2)
    TSC.check_lists(ref, ls, 4, ctx=ctx + " collect", thresholds=False, rows=rows)
    no_overflow(ls, ctx)
    # the COLLECT pass' cand_h: the seed it was given and the query's eps, per list position
    h = ls.host()[2]
    for s in range(S2):
        np.testing.assert_array_equal(h[:, s, 0], hseed.cpu().numpy(), err_msg=ctx)
    TSC.refine_groups(ops, ls, k, ctx, collect=1)


def test_subset_collect(torch_cuda):
    two_pass(torch_cuda, 32, QLIST41, "subset two-pass A=32")


@pytest.mark.parametrize("A", [32, 64])
def test_subset_stream(torch_cuda, A):
    src, ref = GM.data("base", A, 32, 2)
    cap = _lib.lib().dmlp_screen_stream_cap(32)
    for S in (1, 3):
        TSC.three_term(torch_cuda, src, ref, "stream", cap, 32, S, f"subset stream A={A} S={S}",
                       qidx=QLIST)


@pytest.mark.parametrize("cap,kmax", [(128, 32), (512, 256)])
def test_subset_lds(torch_cuda, cap, kmax):
    src, ref = GM.data("base", 32, kmax, 2)
    for S in (1, 3):
        TSC.three_term(torch_cuda, src, ref, "lds", cap, kmax, S, f"subset lds cap={cap} S={S}",
                       qidx=QLIST)


# ================================================================== B. block map
@pytest.mark.parametrize("case", [c for c in GM.X1_CASES if c[0].startswith("xcd")],
                         ids=lambda c: c[0])
def test_xcd_x1(torch_cuda, case):
    """S % 8 == 0 with 3 query blocks (2 for the subset and the empty-slice case): base, ragged
    (the last slice 3 tiles, the last tile 32 padding rows) and empty slices (count 0, eps
    written), then dmlp_refine_groups over all S slices.  (Not on the empty-slice case: its
    one-tile slices hold 8 groups, fewer than most k, so they form no threshold, list every group,
    and the refine rightly hands back the queries whose 300 members exceed its 128 slots.)"""
    ops, ls = x1_and_check(torch_cuda, case)
    if case[1][0] == "empty":
        cnt = ls.host()[1]
        assert (cnt[:, 5:] == 0).all() and (cnt[:, :5] > 0).all()
    else:
        TSC.refine_groups(ops, ls, case[1][2], case[0])


PARTS = {"8+4": (12, [(0, 8), (8, 4)]), "8+8": (16, [(0, 8), (8, 8)]),
         "4..12,0..4,12..16": (16, [(4, 8), (0, 4), (12, 4)])}


@pytest.mark.parametrize("split", list(PARTS))
@pytest.mark.parametrize("kmax", [16, 64])
def test_xcd_x1_parts(torch_cuda, kmax, split):
    """dmlp_screen_x1_part: S_l picks the block decode, S lays out the lists.  The launches of a
    split (XCD-aware ones at S_l = 8, plain ones at S_l = 4, any order) write the lists of one
    dmlp_screen_x1 over all S slices."""
    S, parts = PARTS[split]
    inp, ref = GM.data("base", 32, kmax, 1)
    ops = TSC.Ops(torch_cuda, ref, inp.labels)
    ctx = f"parts {split} kmax={kmax}"
    grows = TSC.grows_of(ops.L, ref, kmax)
    whole = TSC.run_x1(ops, kmax, S)
    TSC.check_lists(ref, whole, grows, ctx=ctx + " whole")
    part = TSC.run_x1(ops, kmax, S, parts=parts)
    TSC.check_lists(ref, part, grows, ctx=ctx + " parts")
    same_lists(whole, part, ctx)


@pytest.mark.parametrize("S", [8, 16])
@pytest.mark.parametrize("kind", ["base", "ragged"])
@pytest.mark.parametrize("impl,cap,kmax", [("stream", 0, 32), ("lds", 128, 32), ("lds", 256, 128)])
def test_xcd_three_term(torch_cuda, impl, cap, kmax, kind, S):
    src, ref = GM.data(kind, 32, kmax, 2)
    cap = cap or _lib.lib().dmlp_screen_stream_cap(kmax)
    TSC.three_term(torch_cuda, src, ref, impl, cap, kmax, S, f"xcd {impl} cap={cap} {kind} S={S}")


# ================================================================== C. scalar k
def part_k_args(ops, ls, kmax, S, s_first, S_l, kuni=-1, qk=None, **over):
    """the arguments of dmlp_screen_x1_part_k, any of KT / hl / A / n_tiles / n_points overridden"""
    r = ops.ref
    a = dict(KT=r.KT, hl=r.hl, A=r.A, n_tiles=r.n_tiles, n_points=r.N)
    a.update(over)
    qk = None if qk is TSC.NULL else ops.qk if qk is None else qk
    return (a["KT"], a["hl"], a["A"], _p(ops.xfrag), _p(ops.xinit), a["n_tiles"], a["n_points"],
            _p(ops.qhi), _p(ops.qn), _p(ops.qidx), _p(qk), kuni, ops.nq, kmax, ops.xnmax, ops.bad,
            S, s_first, S_l, _p(ls.ids), _p(ls.cnt), _p(ls.h), _stream(ops.torch))


@pytest.mark.parametrize("hl,A,kmax", GM.SCALAR_SHAPES)
def test_scalar_k_part(torch_cuda, hl, A, kmax):
    """kuni = kmax with qk null and with qk an array of ones that must not be read: I1 - I5 for
    k = kmax (I3 fails for the lists k = 1 gives) and the lists of the kuni = -1 launch, over all
    rows and over the 77-row list, with the plain block decode (S = 1) and the XCD one (S = 8);
    kuni = kmax + 1 is rejected before any launch."""
    torch = torch_cuda
    inp, ref = GM.data(GM.kind_of(hl, kmax), A, kmax, hl, kmin=kmax)
    assert (ref.k == kmax).all()
    ones = torch.ones(ref.Q, dtype=torch.int32, device="cuda")
    for rows in (None, QLIST):
        ops = TSC.Ops(torch, ref, inp.labels, qidx=rows)
        grows = TSC.grows_of(ops.L, ref, kmax)
        for S in (1, 8):
            ctx = f"scalar k hl={hl} A={A} k={kmax} S={S} {'all' if rows is None else 'subset'}"
            want = TSC.run_x1(ops, kmax, S)
            TSC.check_lists(ref, want, grows, ctx=ctx + " qk", rows=rows)
            for qk in (TSC.NULL, ones):
                ls = TSC.run_x1(ops, kmax, S, qk=qk, kuni=kmax)
                TSC.check_lists(ref, ls, grows, ctx=ctx, rows=rows)
                same_lists(want, ls, ctx)
    ls = TSC.Lists(torch, ops.nq, 8, want.cap)
    assert ops.L.dmlp_screen_x1_part_k(*part_k_args(ops, ls, kmax, 8, 0, 8, kuni=kmax + 1)) == -1
    torch.cuda.synchronize()
    ls.untouched("kuni = kmax + 1")


def test_scalar_k_early(torch_cuda):
    torch = torch_cuda
    hl, A, kmax = 1, 32, 16
    inp, ref = GM.data("base", A, kmax, hl, kmin=kmax)
    ones = torch.ones(ref.Q, dtype=torch.int32, device="cuda")
    for rows in (None, QLIST):
        ops = TSC.Ops(torch, ref, inp.labels, qidx=rows)
        grows = TSC.grows_of(ops.L, ref, kmax)
        ctx = f"scalar k early {'all' if rows is None else 'subset'}"
        want, _ = TSC.run_x1_early(ops, kmax, rdy_tiles=2)
        TSC.check_lists(ref, want, grows, ctx=ctx + " qk", rows=rows)
        for qk in (TSC.NULL, ones):
            ls, estats = TSC.run_x1_early(ops, kmax, rdy_tiles=2, qk=qk, kuni=kmax)
            assert estats[0] == 0 and estats[2] == 0
            TSC.check_lists(ref, ls, grows, ctx=ctx, rows=rows)
            same_lists(want, ls, ctx)
    L, r = ops.L, ref
    ls = TSC.Lists(torch, ops.nq, 1, want.cap)
    bits = TSC.ready_words(r, 2)
    rdy = torch.from_numpy(bits.view(np.int32)).cuda()
    estats = torch.zeros(3, dtype=torch.int32, device="cuda")
    rc = L.dmlp_screen_x1_early_k(r.KT, r.A, _p(ops.xfrag), _p(ops.xinit), r.n_tiles, r.N,
                                  _p(ops.qhi), _p(ops.qn), _p(ops.qidx), None, kmax + 1, ops.nq,
                                  kmax, ops.bad, _p(rdy), 2, len(bits), _p(ls.ids), _p(ls.cnt),
                                  _p(ls.h), _p(estats), _stream(torch))
    assert rc == -1
    torch.cuda.synchronize()
    ls.untouched("early kuni = kmax + 1")
    assert (estats.cpu().numpy() == 0).all()


# ================================================================== D. instantiations
@pytest.mark.parametrize("kind", ["uniform", "adversarial"])
@pytest.mark.parametrize("A,kmax", GM.D_BF16)
def test_bf16_kt4_kt8(torch_cuda, A, kmax, kind):
    """dmlp_screen_x1 on the bf16 image (operands from dmlp_prep_data / dmlp_prep_queries) at
    KT 4 and 8, both buffer depths, then dmlp_refine_groups.  The uniform data has 448 rows, and
    the class kmax 64 screens k in [1, 32] (see D_UNIFORM_N in the model file: at N = 4096 the
    ideal lists themselves exceed the capacity, and at k near 64 more than the refine's 128
    member slots reach its threshold; k = 48 in that class is the adversarial case's)."""
    src, ref = GM.d_bf16_data(kind, A, kmax)
    ops = TSC.Ops(torch_cuda, ref, src.labels)
    ctx = f"bf16 {kind} A={A} kmax={kmax}"
    ls = TSC.run_x1(ops, kmax, 1)
    TSC.check_lists(ref, ls, TSC.grows_of(ops.L, ref, kmax), ctx=ctx)
    no_overflow(ls, ctx)
    TSC.refine_groups(ops, ls, kmax, ctx)


@pytest.mark.parametrize("kind", ["uniform", "adversarial"])
@pytest.mark.parametrize("A,kmax", GM.D_EARLY)
def test_early_kt8_sub32(torch_cuda, A, kmax, kind):
    """dmlp_screen_x1_early at KT 8 (both buffer depths) and at KT 1 with 32-entry buffers."""
    src, ref = GM.d_early_data(kind, A, kmax)
    ops = TSC.Ops(torch_cuda, ref, src.labels)
    ctx = f"early {kind} A={A} kmax={kmax}"
    ls, estats = TSC.run_x1_early(ops, kmax, rdy_tiles=2)
    assert estats[0] == 0 and estats[2] == 0, f"{ctx}: waits {estats[0]}, timeouts {estats[2]}"
    TSC.check_lists(ref, ls, TSC.grows_of(ops.L, ref, kmax), ctx=ctx)
    no_overflow(ls, ctx)
    same_lists(TSC.run_x1(ops, kmax, 1), ls, ctx + " against the plain screen")
    TSC.refine_groups(ops, ls, kmax, ctx)


@pytest.mark.parametrize("A", [64, 256])
def test_collect_kt2_kt8(torch_cuda, A):
    two_pass(torch_cuda, A, None, f"two-pass A={A}")


# ================================================================== E. full slice
def planted_listed(ref, ls, grows, ctx):
    ids, cnt, _ = ls.host()
    rows = np.concatenate([np.arange(8), np.arange(ref.N - 8, ref.N)])
    want = np.unique(X1.group_of_row(rows, grows))
    assert want.max() == (32767 if grows == 8 else 65535) and want.min() == 0
    for p in range(ref.Q):
        gi = X1.entry_group(ids[p, 0, :cnt[p, 0]])
        assert np.isin(want, gi).all(), f"{ctx}: query {p}: planted groups {want.tolist()} not in " \
                                        f"{sorted(gi.tolist())}"


def test_full_slice(torch_cuda):
    """4096 tiles in one slice: the last rows' entries carry group index 32767 from the KT 1
    screens (8-row groups) and 65535 from the COLLECT pass (4-row groups); one tile more is
    rejected by every entry point before it writes."""
    torch = torch_cuda
    inp, ref = GM.full_slice_case()
    ops = TSC.Ops(torch, ref, inp.labels)
    L, r = ops.L, ref
    assert r.n_tiles == 4096 and L.dmlp_screen_x1_min_slices(4096) == 1 \
        and L.dmlp_screen_x1_min_slices(4097) == 2
    for kmax in (16, 64):
        ctx = f"full slice kmax={kmax}"
        grows = TSC.grows_of(L, ref, kmax)
        ls = TSC.run_x1(ops, kmax, 1)
        TSC.check_lists(ref, ls, grows, ctx=ctx)
        no_overflow(ls, ctx)
        planted_listed(ref, ls, grows, ctx)
        TSC.refine_groups(ops, ls, kmax, ctx)
    # the COLLECT pass at the 32-entry screen's thresholds (h <= t - eps by I3: a valid seed)
    hseed = ls.h[0:2 * ops.nq:2].clone().contiguous()
    lc = TSC.run_x1_collect(ops, hseed, 1024, 1)
    TSC.check_lists(ref, lc, 4, ctx="full slice collect", thresholds=False)
    no_overflow(lc, "full slice collect")
    planted_listed(ref, lc, 4, "full slice collect")
    TSC.refine_groups(ops, lc, GM.FULL_K, "full slice collect", collect=1)

    # 4097 tiles (the same buffers: nothing may be launched)
    head = (_p(ops.xfrag), _p(ops.xinit), 4097, r.N, _p(ops.qhi), _p(ops.qn), _p(ops.qidx),
            _p(ops.qk), ops.nq)
    ls = TSC.Lists(torch, ops.nq, 1, L.dmlp_screen_x1_cap_kt(1, 16))
    tail = (_p(ls.ids), _p(ls.cnt), _p(ls.h))
    assert L.dmlp_screen_x1(r.KT, 1, r.A, *head, 16, ops.xnmax, ops.bad, 1, *tail,
                            _stream(torch)) == -4
    assert L.dmlp_screen_x1_collect(r.KT, r.A, *head, ops.xnmax, ops.bad, _p(hseed), ls.cap, 1,
                                    *tail, _stream(torch)) == -4
    rdy = torch.ones(65, dtype=torch.int32, device="cuda")
    estats = torch.zeros(3, dtype=torch.int32, device="cuda")
    assert L.dmlp_screen_x1_early(r.KT, r.A, *head, 16, ops.bad, _p(rdy), 64, 65, *tail,
                                  _p(estats), _stream(torch)) == -1
    torch.cuda.synchronize()
    ls.untouched("4097 tiles")
    assert (estats.cpu().numpy() == 0).all()


# ================================================================== F. argument errors
ERRORS = {
    # name: (expected code, S, s_first, S_l, kmax, overrides)
    "s_first + S_l > S": (-1, 4, 2, 3, 16, {}),
    "s_first < 0": (-1, 4, -1, 2, 16, {}),
    "hl = 3": (-1, 4, 0, 4, 16, dict(hl=3)),
    "KT = 3": (-3, 4, 0, 4, 16, dict(KT=3)),
    "A > 32 KT": (-3, 4, 0, 4, 16, dict(A=33)),
    "kmax = 65": (-3, 4, 0, 4, 65, {}),
    "n_points > 64 n_tiles": (-1, 4, 0, 4, 16, dict(n_points=64 * 64 + 1)),
    "S_l = 0": (0, 4, 2, 0, 16, {}),
}


@pytest.mark.parametrize("name", list(ERRORS))
def test_part_argument_errors(torch_cuda, name):
    """dmlp_screen_x1_part: the code csrc/screen_x1.hip returns for each bad argument, and not a
    word of the lists written (S_l = 0: no slices to do, 0)."""
    code, S, s_first, S_l, kmax, over = ERRORS[name]
    inp, ref = GM.data("base", 32, 16, 1)
    assert ref.n_tiles == 64 and ref.KT == 1
    ops = TSC.Ops(torch_cuda, ref, inp.labels)
    ls = TSC.Lists(torch_cuda, ops.nq, S, 124)
    args = part_k_args(ops, ls, kmax, S, s_first, S_l, **over)
    assert ops.L.dmlp_screen_x1_part(*args[:11], *args[12:]) == code, name
    torch_cuda.cuda.synchronize()
    ls.untouched(name)


# ================================================================== the LDS screen's fp16 form
@pytest.mark.parametrize("S,subset", [(3, True), (8, False)])
def test_screen_lds_fp16(torch_cuda, S, subset):
    """dmlp_screen_hl(hl = 1): the LDS screen's single-term form on the host's fp16 image (no
    caller in the dispatcher today; kept, so tested): complete id lists or overflow, as the 3-term
    form, then dmlp_refine."""
    torch = torch_cuda
    cap, kmax = 128, 32
    src, ref = GM.data("base", 32, kmax, 1)
    rows = QLIST if subset else None
    ops = TSC.Ops(torch, ref, src.labels, qidx=rows)
    L = ops.L
    ctx = f"lds fp16 S={S}"
    assert kmax <= L.dmlp_screen_kmax(cap) and L.dmlp_screen_waves_hl(ref.KT, cap, 1) > 0
    ls = TSC.Lists(torch, ops.nq, S, cap)
    _lib.check(L.dmlp_screen_hl(ref.KT, cap, 1, ref.A, _p(ops.xfrag), _p(ops.xinit), ref.n_tiles,
                                _p(ops.qhi), None, _p(ops.qn), _p(ops.qidx), _p(ops.qk), ops.nq,
                                ops.xnmax, ops.bad, np.float32(0.0), S, _p(ls.ids), _p(ls.cnt),
                                _stream(torch)), "screen_hl")
    torch.cuda.synchronize()
    ls.check_band(ctx)
    ids, cnt, _ = ls.host()
    assert (cnt != -7).all()
    TSC.check_id_lists(ref, ids, cnt, S, ctx, rows=rows)
    assert (cnt < 0).sum() <= 0.05 * cnt.size, f"{ctx}: {(cnt < 0).sum()} of {cnt.size} overflowed"
    out = TSC.Out(torch, ref.Q, kmax)
    _lib.check(L.dmlp_refine(cap, _p(ls.ids), _p(ls.cnt), S, _p(ops.X), ref.A, _p(ops.Qx),
                             _p(ops.qidx), _p(ops.qk), ops.nq, _p(out.d), _p(out.i), out.kstride,
                             *TSC._label_args(ops, out, True), _p(out.status), _p(out.ovf),
                             _stream(torch)), "refine")
    TSC.check_refined(ops, out, True, ctx + " refine", handed_back=(cnt < 0).any(axis=1), rows=rows)
