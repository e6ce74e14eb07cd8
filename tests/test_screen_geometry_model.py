"""The screens' launch geometry: the cases of tests/test_screen_geometry.py and, on the CPU, the proof
that the generalised checker sees what those cases are for.

The contract tests of tests/test_screen_contract.py run every screen with qidx = arange(Q) and
S <= 5.  Production hands the screens an unsorted class subset (the kernels index the lists, hseed
and cand_h by list position p, the operands, qn and qk by row q = qidx[p]) and S % 8 == 0 (the
XCD-aware decode of blockIdx.x).  This file defines the data and the case lists both files use
(the GPU file imports it) and shows, with no GPU:

  * check_lists(rows=...) accepts the ideal lists of the float64 reference (ModelLists of
    tests/test_screen_x1_schedule.py, told which row each position holds) for every single-term
    case, and those lists keep at most cap - 4 entries per (p, s): the condition behind "no count
    is -1" in the GPU cases;
  * check_lists rejects each mutant of those lists that a p / q mix-up, a wrong block decode, a
    stale k or a truncated group index would write.  A mutant is asserted on every case it applies
    to, so a case whose data could not tell the difference fails here, not silently on the GPU.
"""
import functools
import os
import sys

import numpy as np
import pytest

import distributed_machine_learning_project_amd as dmlp

HERE = os.path.dirname(os.path.abspath(__file__))
for _d in (HERE, os.path.join(HERE, "helpers")):
    if _d not in sys.path:
        sys.path.insert(0, _d)
import test_screen_contract as TSC  # noqa: E402  (uniform_case, check_lists)
import test_screen_x1_schedule as SCH  # noqa: E402  (ModelLists, grows_for, cap_for)
import x1_contract as X1  # noqa: E402

# ------------------------------------------------------------------ the query lists
# 77 of the 130 rows, unsorted: a full x1 workgroup and a second one of 13 columns (4 full waves
# and 13 columns of a fifth for the 16-column screens)
QLIST = np.random.default_rng(4).permutation(130)[:77].astype(np.int32)
# 41 of the two-pass case's 70 rows
QLIST41 = np.random.default_rng(4).permutation(70)[:41].astype(np.int32)
assert (np.diff(QLIST) < 0).any() and (np.diff(QLIST41) < 0).any()


# ------------------------------------------------------------------ data (built once, shared)
def data(kind: str, A: int, kmax: int, hl: int, kmin: int = 1):
    """base: N = 4096 (64 tiles), Q = 130 (3 x1 workgroups per slice), k mixed in [kmin, kmax];
    ragged: N = 4000 (63 tiles: with S = 16 the last slice has 3 tiles, the last tile 32 padding
    rows); empty: N = 300, Q = 70 (5 tiles: with S = 8 slices 5 - 7 are empty); small: N = 1024
    (16 tiles), for the bf16 image's classes kmax 32 and 64 — its eps is 8 times the fp16 image's,
    and at N = 4096 a compaction of those classes can keep up to 60 and 125 entries, more than the
    56 and 120 the lists hold (worst_kept below; the kernel then reports overflow, rightly)."""
    kw = {"base": {}, "ragged": dict(N=4000), "empty": dict(N=300, Q=70), "small": dict(N=1024)}[kind]
    return TSC.uniform_case(A, kmax, hl, kmin=kmin, **kw)


def kind_of(hl, kmax):
    """the data of a subset or scalar-k case"""
    return "small" if hl == 2 and kmax > 16 else "base"


FULL_N, FULL_Q, FULL_K = 4096 * 64, 5, 16


@functools.lru_cache(maxsize=None)
def full_slice_case():
    """One slice of 4096 tiles, the most an entry's 16-bit group index can address: uniform rows,
    except that the last 8 rows are the 8 nearest of every query and rows 0 - 7 the next 8 (their
    entries carry the largest and the smallest group index of the slice).  k = 16 everywhere."""
    N, Q, A, k = FULL_N, FULL_Q, 32, FULL_K
    inp = dmlp.generate(N, Q, A, 0.0, 1000.0, k, k, 10, seed=65535)
    X, Qx = inp.X.copy(), inp.Qx.copy()
    g = np.random.default_rng(65536)
    q6 = lambda x: np.rint(np.asarray(x) * 1.0e6) / 1.0e6
    cen = np.full(A, 500.0)
    sign = np.where(np.arange(A) & 1, -1.0, 1.0)
    X[N - 8:] = q6(cen + g.uniform(-1.0, 1.0, (8, A)))              # |x - q| <= 1.5 per attribute
    X[:8] = q6(cen + 4.0 * sign + g.uniform(-0.5, 0.5, (8, A)))     # in [3, 5] per attribute
    Qx = q6(cen + g.uniform(-0.5, 0.5, (Q, A)))
    inp = type(inp)(inp.labels, np.ascontiguousarray(X), inp.k, np.ascontiguousarray(Qx))
    ref = X1.reference(inp.X, inp.Qx, inp.k, hl=1)
    for q in range(Q):
        assert sorted(ref.nn_i[q, :8].tolist()) == list(range(N - 8, N))
        assert sorted(ref.nn_i[q, 8:16].tolist()) == list(range(8))
    return inp, ref


# ------------------------------------------------------------------ the single-term cases
# (name, (kind, A, kmax, hl, kmin), S, rows): every dmlp_screen_x1 geometry of the GPU file's
# sections A (query subsets), B (block map) and C (scalar k; kmin = kmax)
SUBSET_SHAPES = [(1, 32, 16), (1, 64, 64), (2, 32, 32), (2, 64, 64)]       # (hl, A, kmax)
XCD_SHAPES = [(hl, 32, kmax) for kmax in (16, 64) for hl in (1, 2)]
SCALAR_SHAPES = [(1, 32, 16), (2, 64, 64)]


def x1_cases():
    out = []
    for hl, A, kmax in SUBSET_SHAPES:
        out += [(f"subset hl={hl} A={A} kmax={kmax} S={S}", (kind_of(hl, kmax), A, kmax, hl, 1), S, QLIST)
                for S in (1, 4)]
    for hl, A, kmax in XCD_SHAPES:
        out += [(f"xcd hl={hl} kmax={kmax} S={S}", ("base", A, kmax, hl, 1), S, None)
                for S in (8, 16)]
        out.append((f"xcd ragged hl={hl} kmax={kmax} S=16", ("ragged", A, kmax, hl, 1), 16, None))
        out.append((f"xcd empty hl={hl} kmax={kmax} S=8", ("empty", A, kmax, hl, 1), 8, None))
    for kmax in (16, 64):       # the part launches' S (8 + 4; 16 is above)
        out.append((f"parts kmax={kmax} S=12", ("base", 32, kmax, 1, 1), 12, None))
    out.append(("xcd subset S=16", ("base", 32, 16, 1, 1), 16, QLIST))
    for hl, A, kmax in SCALAR_SHAPES:
        for S in (1, 8):
            for rows in (None, QLIST):
                out.append((f"scalar hl={hl} A={A} k={kmax} S={S} {'all' if rows is None else 'subset'}",
                            (kind_of(hl, kmax), A, kmax, hl, kmax), S, rows))
    return out


X1_CASES = x1_cases()


def by_name(name):
    return next(c for c in X1_CASES if c[0] == name)


def model(case, **kw):
    """(ref, grows, cap, the ideal lists) of one case; kw: ModelLists' mutation switches"""
    name, dat, S, rows = case
    _, ref = data(*dat)
    kmax = dat[2]
    grows, cap = SCH.grows_for(ref, kmax), SCH.cap_for(kmax)
    return ref, grows, cap, SCH.ModelLists(ref, S, cap, grows, rows=rows, **kw)


def worst_kept(ref, S, grows, rows=None, k=None):
    """An upper bound on the entries any compaction of k_screen_x1 can keep for a (p, s) of this
    case: over every prefix of the slice's scan (whole append rounds: 4 group entries), the groups
    seen so far whose key reaches key(ak - 2 eps) - 1, with ak decoded from the k-th largest key
    seen with its low bit dropped (the kernel's 15-bit radix select), eps raised by I1's rtol, and
    one key of slack for the MFMA's accumulation order.  The thresholds only rise, so what a
    compaction keeps is a subset of this whatever the compactions before it did.  At or below
    cap - 4 (CAPE), no compaction overflows: every count the kernel writes is >= 0."""
    rows = np.arange(ref.Q) if rows is None else np.asarray(rows, np.int64)
    kk = np.asarray(ref.k if k is None else k)[rows].astype(np.int64)
    eps = ref.eps[rows].astype(np.float32) * np.float32(1.0 + 1.0e-5)
    tps = X1.tiles_per_slice(ref.n_tiles, S)
    lowest = np.float32(-np.finfo(np.float32).max)
    ar, worst = np.arange(len(rows)), 0
    for s in range(S):
        r0, r1 = X1.slice_rows(ref.n_tiles, S, s, ref.N)
        nts = max(0, min((s + 1) * tps, ref.n_tiles) - s * tps)
        if nts == 0:
            continue
        gm = X1.group_max(ref.a_model[rows][:, r0:r1].astype(np.float32), nts, grows)
        real = gm > -np.inf
        keys = np.where(real, X1.key16(np.where(real, gm, 0.0).astype(np.float32)), -1)
        for L in range(4, keys.shape[1] + 1, 4):
            kl = keys[:, :L]
            sel = (kk >= 1) & ((kl >= 0).sum(axis=1) >= kk)
            kth = np.sort(kl, axis=1)[ar, np.clip(L - kk, 0, L - 1)]
            ak = X1.decode16(np.where(sel, kth & ~1, 0)).astype(np.float32)
            thr = np.where(sel, X1.key16(np.maximum(lowest, ak - np.float32(2.0) * eps)) - 1, 0)
            worst = max(worst, int(((kl >= thr[:, None]) & (kl >= 0)).sum(axis=1).max()))
    return worst


class HostLists:
    """lists edited on the host (the mutants)"""

    def __init__(self, ls):
        self.S, self.cap = ls.S, ls.cap
        self.ids, self.cnt, self.h = (a.copy() for a in ls.host())

    def host(self):
        return self.ids, self.cnt, self.h


def check(case, ls, ref, grows, k=None):
    TSC.check_lists(ref, ls, grows, k=k, ctx=case[0], rows=case[3])


def rejected(case, ls, ref, grows, k=None):
    with pytest.raises(AssertionError):
        check(case, ls, ref, grows, k=k)


# ------------------------------------------------------------------ the checker accepts the ideal lists
@pytest.mark.parametrize("case", X1_CASES, ids=lambda c: c[0])
def test_ideal_lists_accepted(case):
    """I1 - I5 with rows, and at most cap - 4 kept entries per (p, s), in the ideal lists and in
    any compaction on the way to them: no GPU case can overflow."""
    ref, grows, cap, ls = model(case)
    check(case, ls, ref, grows)
    assert ls.cnt.max() <= cap - 4, f"{case[0]}: the ideal lists keep {ls.cnt.max()} > cap - 4"
    worst = worst_kept(ref, case[2], grows, rows=case[3])
    assert ls.cnt.max() <= worst <= cap - 4, f"{case[0]}: a compaction may keep {worst} > cap - 4"
    if case[1][0] == "empty":
        assert (ls.cnt[:, 5:] == 0).all() and (ls.cnt[:, :5] > 0).all()


# ------------------------------------------------------------------ instantiations (section D)
# The bf16 image at KT 4 and 8.  Uniform rows in 128 or 256 dimensions have scores so close
# together, measured in the bf16 bound's eps, that at N = 4096 the ideal lists of the classes
# kmax 32 and 64 keep up to 90 and 160 entries, more than cap - 4 = 56 and 120.  The uniform data of
# these cases therefore has N = 448 rows (7 tiles): 56 8-row groups or 112 4-row groups, which no
# list can overflow, while the threshold still drops up to half of them.  The group refine has 128
# member slots and hands a query back when more members reach its threshold; at k near 64 up to
# 150 of these rows do (refine_survivors below), so the class kmax 64 screens the queries of the
# class kmax 32 (k mixed in [1, 32]); k = 48 in that class is the adversarial case's.
D_UNIFORM_N = 448
D_BF16 = [(A, kmax) for A in (128, 256) for kmax in (16, 32, 64)]
D_EARLY = [(256, 16), (256, 64), (32, 64)]


def d_bf16_data(kind, A, kmax):
    if kind == "uniform":
        return TSC.uniform_case(A, min(kmax, 32), 2, N=D_UNIFORM_N)
    return TSC.adv_case("normal", 2, A, kmax, "one")


def refine_survivors(ref, grows):
    """An upper bound on the members the group refine keeps per query of a one-slice case: the
    rows whose score reaches ak - 2 eps, with ak from the k-th largest group key with its low bit
    dropped, eps raised by I1's rtol and 2^-20 |h| for the accumulation order."""
    keys = X1.key16(X1.group_max(ref.a_model.astype(np.float32), ref.n_tiles, grows))
    kth = np.sort(keys, axis=1)[np.arange(ref.Q), keys.shape[1] - ref.k.astype(np.int64)]
    h = X1.decode16(kth & ~1) - 2.0 * ref.eps.astype(np.float64) * (1.0 + 1.0e-5)
    h -= np.abs(h) * 2.0 ** -20
    return int((ref.a_model >= h[:, None]).sum(axis=1).max())


def d_early_data(kind, A, kmax):
    return TSC.uniform_case(A, kmax, 1) if kind == "uniform" else TSC.adv_case("normal", 1, A, kmax, "one")


@pytest.mark.parametrize("kind", ["uniform", "adversarial"])
@pytest.mark.parametrize("form,A,kmax", [("bf16",) + c for c in D_BF16] + [("early",) + c for c in D_EARLY])
def test_instantiation_cases_fit(form, A, kmax, kind):
    """adversarial_normal builds at every A of section D; the ideal lists of its cases satisfy
    I1 - I5 and fit the lists."""
    early = form == "early"
    _, ref = (d_early_data if early else d_bf16_data)(kind, A, kmax)
    assert ref.KT == {32: 1, 128: 4, 256: 8}[A]
    grows, cap = SCH.grows_for(ref, kmax), SCH.cap_for(kmax)
    ls = SCH.ModelLists(ref, 1, cap, grows)
    TSC.check_lists(ref, ls, grows, ctx=f"{kind} A={A} kmax={kmax}")
    assert ls.cnt.max() <= worst_kept(ref, 1, grows) <= cap - 4
    if not early:
        assert refine_survivors(ref, grows) <= 112, "dmlp_refine_groups would hand a query back"
    if kind == "uniform" and not early:
        assert X1.n_groups(ref.n_tiles, grows) <= cap - 4
        kept = ls.cnt[:, 0] / X1.n_groups(ref.n_tiles, grows)
        assert kept.min() < 0.5, "the threshold must still drop groups"


def test_full_slice_ideal_lists():
    """The full slice: the planted groups carry the slice's largest and smallest group index, in
    the 8-row geometry the KT 1 screens write (32767) and in the COLLECT pass' 4-row one (65535)."""
    _, ref = full_slice_case()
    last, first = np.arange(FULL_N - 8, FULL_N), np.arange(8)
    for grows, top in ((8, 32767), (4, 65535)):
        assert X1.group_of_row(last, grows).max() == top and X1.group_of_row(first, grows).min() == 0
        for kmax in (16, 64):
            cap = SCH.cap_for(kmax)
            ls = SCH.ModelLists(ref, 1, cap, grows)
            TSC.check_lists(ref, ls, grows, ctx=f"full slice grows={grows} kmax={kmax}")
            assert ls.cnt.max() <= cap - 4
            for p in range(FULL_Q):
                gi = X1.entry_group(ls.ids[p, 0, :ls.cnt[p, 0]])
                assert np.isin(X1.group_of_row(np.concatenate([first, last]), grows), gi).all()


# ------------------------------------------------------------------ the checker rejects the mutants
SUBSET_CASES = [c for c in X1_CASES if c[3] is not None and c[1][4] == 1]      # mixed k, a subset
XCD16 = [c for c in X1_CASES if c[2] == 16 and c[3] is None]
EMPTY_CASES = [c for c in X1_CASES if c[1][0] == "empty"]
SCALAR_CASES = [c for c in X1_CASES if c[0].startswith("scalar")]
_ids = lambda c: c[0]


@pytest.mark.parametrize("case", SUBSET_CASES, ids=_ids)
def test_mutant_eps_of_position(case):
    """eps from qn[p] instead of qn[qidx[p]]: I1 (the norms differ per query by far more than its
    rtol), whether or not the threshold moved enough for I3."""
    ref, grows, cap, ls = model(case, eps_rows=np.arange(len(case[3])))
    assert not np.allclose(ref.eps[case[3]], ref.eps[:len(case[3])], rtol=1e-3)
    rejected(case, ls, ref, grows)


@pytest.mark.parametrize("case", SUBSET_CASES, ids=_ids)
def test_mutant_k_of_position(case):
    """k from qk[p] instead of qk[qidx[p]]: where k[p] < k[q] the threshold is too high (I3) or a
    neighbour is dropped (I2)."""
    ref, grows, cap, ls = model(case, k_rows=np.arange(len(case[3])))
    assert (ref.k[:len(case[3])] < ref.k[case[3]]).any()
    rejected(case, ls, ref, grows)


@pytest.mark.parametrize("case", SUBSET_CASES, ids=_ids)
def test_mutant_list_at_row(case):
    """the lists of position p stored at row qidx[p] (what lands inside the nq positions; the
    rest would fall into the sentinel band or past it)."""
    ref, grows, cap, ideal = model(case)
    rows, S = case[3], case[2]
    ids = np.zeros((ref.Q, S, cap), np.int64)
    cnt = np.full((ref.Q, S), -7, np.int32)
    h = np.full((ref.Q, S, 2), np.nan, np.float32)
    ids[rows], cnt[rows], h[rows] = ideal.ids, ideal.cnt, ideal.h
    ls = HostLists(ideal)
    ls.ids, ls.cnt, ls.h = ids[:len(rows)], cnt[:len(rows)], h[:len(rows)]
    rejected(case, ls, ref, grows)
    # ... and with every position written (a permutation of the lists among the positions)
    ls = HostLists(ideal)
    perm = np.argsort(np.argsort(rows))
    ls.ids, ls.cnt, ls.h = ideal.ids[perm], ideal.cnt[perm], ideal.h[perm]
    rejected(case, ls, ref, grows)


@pytest.mark.parametrize("swap", [(1, 8), (0, 1), (7, 8), (14, 15)])
@pytest.mark.parametrize("case", XCD16, ids=_ids)
def test_mutant_slices_swapped(case, swap):
    """two slices' lists swapped within every query: a wrong xcd * m + sl decode.  (1, 8) is what
    s = sl * 8 + xcd would do to S = 16.)"""
    ref, grows, cap, ideal = model(case)
    a, b = swap
    ls = HostLists(ideal)
    for arr in (ls.ids, ls.cnt, ls.h):
        arr[:, [a, b]] = arr[:, [b, a]]
    rejected(case, ls, ref, grows)


@pytest.mark.parametrize("case", [c for c in X1_CASES if c[2] in (8, 16) and c[3] is None
                                  and c[1][0] != "empty"], ids=_ids)
def test_mutant_query_blocks_swapped(case):
    """the first two workgroups' columns swapped within one slice: a wrong local / n_qblocks
    decode (Q = 130: blocks of 64, 64 and 2 columns)."""
    ref, grows, cap, ideal = model(case)
    for s in (0, case[2] - 1):
        ls = HostLists(ideal)
        for arr in (ls.ids, ls.cnt, ls.h):
            arr[:128, s] = np.concatenate([arr[64:128, s], arr[:64, s]])
        rejected(case, ls, ref, grows)


@pytest.mark.parametrize("case", X1_CASES, ids=_ids)
def test_mutant_cell_unwritten(case):
    """one (p, s) cell left at its sentinel: the last position of the last slice"""
    ref, grows, cap, ideal = model(case)
    ls = HostLists(ideal)
    ls.cnt[-1, -1] = -7
    ls.h[-1, -1] = np.nan
    rejected(case, ls, ref, grows)


@pytest.mark.parametrize("case", EMPTY_CASES, ids=_ids)
def test_mutant_empty_slice_unwritten(case):
    """an empty slice (no tiles) must report count 0 and the query's eps, not stay unwritten"""
    ref, grows, cap, ideal = model(case)
    ls = HostLists(ideal)
    ls.cnt[:, 5:] = -7
    rejected(case, ls, ref, grows)
    ls = HostLists(ideal)
    ls.h[:, 5:, 1] = np.nan       # (the count written, cand_h not: I1)
    rejected(case, ls, ref, grows)


@pytest.mark.parametrize("case", SCALAR_CASES, ids=_ids)
def test_mutant_k1_under_scalar_k(case):
    """the lists k = 1 gives (the qk array of ones that must not be read) judged for k = kmax"""
    ref, grows, cap, _ = model(case)
    assert (ref.k == case[1][2]).all()
    ls = SCH.ModelLists(ref, case[2], cap, grows, rows=case[3], k=np.ones(ref.Q, np.int32))
    rejected(case, ls, ref, grows)


def test_mutant_group_index_15_bits():
    """group index 65535 truncated to 15 bits (the COLLECT pass' 4-row groups on the full slice):
    the last rows' groups are listed under the indices of rows far away."""
    _, ref = full_slice_case()
    ideal = SCH.ModelLists(ref, 1, SCH.cap_for(16), 4)
    ls = HostLists(ideal)
    gi = X1.entry_group(ls.ids)
    assert gi.max() == 65535
    ls.ids = (ls.ids & ~np.int64(0xFFFF)) | (gi & 0x7FFF)
    with pytest.raises(AssertionError):
        TSC.check_lists(ref, ls, 4, ctx="15-bit group index")
