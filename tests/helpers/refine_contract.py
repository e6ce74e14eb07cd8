"""Hand-built candidate lists for the refine kernels (csrc/refine.hip, csrc/refine_pair.hip) and the
float64 reference of what a refine must write for them.  NumPy and the CPU side of libdmlp only: no GPU.

The screens list generously, so on their lists most of the refine's rule cannot be seen: a
dropped non-neighbour changes nothing.  Here the lists are written by hand — which groups, in
which order, how many, which threshold — so that every branch of the rule decides the answer.

The rule (refine.hip k_refine / refine_pair.hip k_refine_pair), per listed query p of row q:
  overflow   a slice count of -1 -> status 1
  threshold  one slice, not collect: hq = cand_h[p][0][0]; collect: hq starts at slice 0's seed;
             S > 1 or collect, and M >= k >= 1 (M: listed entries): hq = max(hq, decode16(k-th
             largest key, with multiplicity) - 2 max_s eps_s) in fp32; else S > 1: hq = -inf
  survivors  an entry is live iff key >= key16(hq); a member row of a live entry survives iff its
             global row (slice * tiles_per_slice * 64 + group row) is < n_points and, with an image,
             its single-term score reaches hq (without: every member survives)
  hand-back  more survivors than the kernel's member slots -> status 1
  status 0   slots [0, min(k, survivors)) = the survivors' exact top-k (left-to-right fp64 distance,
             (dist asc, id desc)), the rest of [0, kstride) = (+inf, -1); label and checksum of that
             list
  status 1   slots [0, k) untouched, [k, kstride) = (+inf, -1); label and checksum untouched;
             *ovf_count grows by one
  dmlp_refine reads plain global row ids: no threshold, no member limit.

The kernels sum the score in fp32, a_model is the float64 value of the same operands; they differ
by less than the query's eps.  Every case therefore keeps every listed member's score further
than MARGIN * eps from the threshold in force (asserted in Builder.done): that margin is the only
tolerance, everything else the tests compare is bits and integers.

Slots past a count hold entries that must never be read: the query's nearest groups (rows) of
that slice that are not listed, with key 0xFFFF.  A kernel that reads them writes a nearer list.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field, replace

import numpy as np

import result_contract as RC
import x1_contract as X1
from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.ops import knn as K

MARGIN = 1.01            # of eps, between every listed member's score and the threshold
PAIR_MEMBERS, GROUP_MEMBERS, BIG_MEMBERS = 64, 128, 512   # PM; P of k_refine<2, KT>; of <8, KT>
S_MAX = 256
NEAR_P = 112             # near-tie rows: N = RC.N_FILL + NEAR_P = 2112


# ------------------------------------------------------------------ the rule and its mutants
@dataclass(frozen=True)
class Rule:
    cap_delta: int = 0          # member slots off by this
    threshold: bool = True      # False: every member of every entry survives
    two_eps: bool = True        # False: the global threshold without the - 2 eps
    eps_slice0: bool = False    # eps of slice 0 instead of the largest
    kth_distinct: bool = False  # the k-th largest DISTINCT key
    cut: bool = True            # False: rows >= n_points are members too
    to_cap: bool = False        # entries read up to cap instead of the count
    swap_grows: bool = False    # 4-row geometry where 8-row is meant and the reverse
    r2l: bool = False           # distance summed from the last attribute down
    id_asc: bool = False        # ties by ascending id


RULE = Rule()
MUTANTS = {
    "cap_minus": Rule(cap_delta=-1), "cap_plus": Rule(cap_delta=1),
    "no_threshold": Rule(threshold=False), "no_2eps": Rule(two_eps=False),
    "eps_slice0": Rule(eps_slice0=True), "kth_distinct": Rule(kth_distinct=True),
    "no_cut": Rule(cut=False), "to_cap": Rule(to_cap=True), "swap_grows": Rule(swap_grows=True),
    "r2l": Rule(r2l=True), "id_asc": Rule(id_asc=True),
}


def threshold(keys, h, k: int, S: int, collect: bool, rule: Rule = RULE):
    """hq (fp32) of one query: keys of its listed entries, h [S, 2] = cand_h."""
    ninf = np.float32(-np.inf)
    if not rule.threshold:
        return ninf
    hq = np.float32(h[0, 0]) if (S == 1 or collect) else ninf
    if (S > 1 or collect) and len(keys) >= k >= 1:
        srt = np.sort(np.unique(keys) if rule.kth_distinct else np.asarray(keys))[::-1]
        kth = srt[min(k, len(srt)) - 1]
        eps = np.float32(h[0, 1]) if rule.eps_slice0 else np.float32(h[:, 1].max())
        with np.errstate(over="ignore"):
            t = np.float32(X1.decode16(kth))
            if rule.two_eps:
                t = np.float32(t - np.float32(2.0) * eps)
        hq = max(hq, t)
    return np.float32(hq)


def survivors(ent, cnt, h, k: int, n_points: int, tps: int, grows: int, collect: bool = False,
              score=None, rule: Rule = RULE):
    """(rows, hq) of one query, or (None, None) when a slice overflowed.  ent [S, cap] entries,
    cnt [S], h [S, 2]; score [n_points] float64 (None: no image, every member of a live entry
    survives).  rows: the surviving global rows in candidate order."""
    S, cap = ent.shape
    if (np.asarray(cnt) < 0).any():
        return None, None
    n_read = [cap if rule.to_cap else int(cnt[s]) for s in range(S)]
    e = np.concatenate([ent[s, :n_read[s]] for s in range(S)]).astype(np.int64) & 0xFFFFFFFF
    sl = np.concatenate([np.full(n_read[s], s, np.int64) for s in range(S)])
    key = e >> 16
    hq = threshold(key, np.asarray(h), k, S, collect, rule)
    live = key >= X1.key16(np.array([hq], np.float32))[0]
    g = 12 - grows if rule.swap_grows else grows
    rows = sl[live, None] * tps * 64 + X1.group_rows(e[live] & 0xFFFF, g)
    rows = rows.reshape(-1)
    real = rows < n_points
    keep = real.copy()
    if score is not None and rule.threshold:
        keep[real] = np.asarray(score)[rows[real]] >= np.float64(hq)
    if not rule.cut:   # a padding row scores -inf: it survives only a threshold of -inf
        keep |= ~real & (score is None or hq == -np.inf)
    return rows[keep], hq


def refine_status(e_lists, cnt, h, k: int, N: int, tps: int, grows: int = 4,
                  capacity: int = BIG_MEMBERS, collect: bool = False, score=None) -> int:
    """The hand-back decision alone: 1 for an overflowed slice or more than `capacity` survivors."""
    rows, _ = survivors(np.asarray(e_lists), cnt, h, k, N, tps, grows, collect, score)
    return 1 if rows is None else int(len(rows) > capacity)


def rank(q, X, rows, k: int, kstride: int, rule: Rule = RULE):
    """(dist [kstride], ids [kstride]) of the rows' exact top-k, padded with (+inf, -1)."""
    rows = np.unique(np.asarray(rows, np.int64))            # ascending: topk_ref's tie rule holds
    if rows.size and rows.max() >= len(X):                  # (mutants only) padding rows are zeros
        X = np.vstack([X, np.zeros((rows.max() + 1 - len(X), X.shape[1]))])
    with np.errstate(over="ignore"):
        d = (RC.dist_r2l if rule.r2l else RC.dist_l2r)(q, X[rows])
    od = np.full(kstride, np.inf)
    oi = np.full(kstride, -1, np.int32)
    if rule.id_asc:
        order = np.lexsort((rows, d))[:max(0, min(k, len(rows)))]
        od[:len(order)], oi[:len(order)] = d[order], rows[order]
        return od, oi
    td, ti = RC.topk_ref(d, k, kstride)
    real = ti >= 0
    od[real], oi[real] = td[real], rows[ti[real]]
    return od, oi


# ------------------------------------------------------------------ operands (CPU side)
@dataclass
class Problem:
    key: tuple
    X: np.ndarray
    Qx: np.ndarray
    hl: int                      # 0: no image
    ref: X1.Ref | None
    score: np.ndarray            # [Q, N]: a_model, or (no image) minus the exact distance
    eps: np.ndarray              # fp32 [Q] (zeros without an image)

    N = property(lambda self: self.X.shape[0])
    Q = property(lambda self: self.Qx.shape[0])
    A = property(lambda self: self.X.shape[1])
    KT = property(lambda self: K.screen_kt(self.X.shape[1]))


TIE0, TIE1 = 128, 256      # rows [TIE0, TIE1) of the uniform problems are one row, queries 0 and 1 equal it


@functools.lru_cache(maxsize=None)
def problem(kind: str, A: int, N: int = 0, hl: int = 1) -> Problem:
    """uni:   N uniform 6-decimal rows in [0, 1000), 70 queries; rows [128, 256) identical and
              query 0 on them; image kind hl.
    near:  RC.near_tie_input(A, 112): N = 2112, query 0 constant, rows [1000, 1112) near-tied.
    plain: uni without an image, rows 7, N // 2 and N - 2 at distance +inf (1e200)."""
    if kind == "near":
        X, Qx, b0 = RC.near_tie_input(A, NEAR_P)
        assert b0 == 1000 and X.shape[0] == RC.N_FILL + NEAR_P
    else:
        rng = np.random.default_rng(1000 * A + N)
        X = np.round(rng.uniform(0.0, 1000.0, (N, A)), 6)
        Qx = np.round(rng.uniform(0.0, 1000.0, (70, A)), 6)
        X[TIE0:TIE1] = X[TIE0]
        Qx[0] = Qx[1] = X[TIE0]
        if kind == "plain":
            X[[7, N // 2, N - 2], A // 2] = 1e200
    X, Qx = np.ascontiguousarray(X), np.ascontiguousarray(Qx)
    if kind == "plain":
        with np.errstate(over="ignore"):
            score = -np.stack([RC.dist_l2r(q, X) for q in Qx])
        return Problem((kind, A, N, 0), X, Qx, 0, None, score, np.zeros(len(Qx), np.float32))
    ref = X1.reference(X, Qx, np.ones(len(Qx), np.int32), hl=hl)
    return Problem((kind, A, N, hl), X, Qx, hl, ref, ref.a_model, ref.eps)


def image_scores(ref: X1.Ref):
    """a_model recomputed from the words the kernels read (hl = 1): the tile image xhi (point p's
    8-element chunk f at 16-byte index tile 256 KT + ((p & 63) >> 4) 64 KT + (f >> 2) 64 +
    16 (f & 3) + (p & 15)), xinit and the query fragments qhi."""
    KT, N = ref.KT, ref.N
    xh = ref.xhi.view(np.float16).reshape(-1, 8)
    p = np.arange(N)
    img = np.zeros((N, KT * 32))
    for f in range(4 * KT):
        idx = (p >> 6) * (4 * KT * 64) + (((p & 63) >> 4) * KT + (f >> 2)) * 64 + 16 * (f & 3) + (p & 15)
        img[:, 8 * f:8 * f + 8] = xh[idx].astype(np.float64)
    return ref.qhi.view(np.float16).astype(np.float64) @ img.T + ref.xinit[:N].astype(np.float64)


class Groups:
    """The group entries of every slice of one layout: rows, real rows and each query's group
    maximum of the fp32 score."""

    def __init__(self, prob: Problem, S: int, grows: int, tps: int | None = None):
        self.prob, self.S, self.grows = prob, S, grows
        N = prob.N
        self.n_tiles = (N + 63) // 64
        self.tps = X1.tiles_per_slice(self.n_tiles, S) if tps is None else tps
        self.rows, self.real, self.gmax = [], [], []
        s32 = prob.score.astype(np.float32)
        for s in range(S):
            nts = max(0, min((s + 1) * self.tps, self.n_tiles) - s * self.tps)
            ng = X1.n_groups(nts, grows)
            rows = s * self.tps * 64 + X1.group_rows(np.arange(ng), grows)
            real = rows < N
            gm = np.full((prob.Q, ng), -np.inf, np.float32)
            if ng:
                sc = np.where(real[None], s32[:, np.minimum(rows, N - 1)], np.float32(-np.inf))
                gm = sc.max(axis=2)
            self.rows.append(rows)
            self.real.append(real)
            self.gmax.append(gm)

    def n_real(self, s):
        return self.real[s].sum(axis=1)

    def best(self, q, s, n=None, full=True, exclude=()):
        """group indices of slice s by descending maximum for query q (full: all rows real)"""
        order = np.argsort(-self.gmax[s][q], kind="stable")
        ok = self.n_real(s)[order] == self.grows if full else self.n_real(s)[order] > 0
        order = order[ok & ~np.isin(order, exclude)]
        return order if n is None else order[:n]

    def with_real(self, s, n):
        """a group of slice s with exactly n real rows"""
        g = np.nonzero(self.n_real(s) == n)[0]
        assert len(g), f"no group with {n} real rows (N = {self.prob.N}, {self.grows}-row groups)"
        return int(g[-1])

    def of_rows(self, s, rows):
        """groups of slice s that hold the global rows, in the rows' order, without repeats"""
        g = X1.group_of_row(np.asarray(rows, np.int64) - s * self.tps * 64, self.grows)
        return np.array(list(dict.fromkeys(g.tolist())), np.int64)


# ------------------------------------------------------------------ kernel variants
@dataclass(frozen=True)
class Variant:
    entry: str        # "rm", "groups", "groups2", "exact", "refine"
    capacity: int | None
    kmax: int
    collect: bool = False
    image: bool = True


VARIANTS = {
    "pair": Variant("rm", PAIR_MEMBERS, 32),                   # k_refine_pair<KT>
    "rm64": Variant("rm", GROUP_MEMBERS, 64),                  # k_refine<2, KT> behind _rm
    "groups": Variant("groups", GROUP_MEMBERS, 64),            # k_refine<2, KT>, the 32-entry cap
    "groups16": Variant("groups", GROUP_MEMBERS, 32),          # ... the 16-entry screen's cap
    "groups2": Variant("groups2", GROUP_MEMBERS, 64),
    "collect": Variant("groups2", BIG_MEMBERS, 256, collect=True),   # k_refine<8, KT, true>
    "exact": Variant("exact", BIG_MEMBERS, 256, image=False),        # k_refine<8, 1, true>
    "refine": Variant("refine", None, 128, image=False),             # k_refine<4 | 8, 0>
}
BIG_CAP = 160     # id stride of the hand-built collect / exact lists


def layout(variant: str, KT: int):
    """(cap, rows per group) of a variant's lists, as its producing screen states them."""
    v = VARIANTS[variant]
    if v.collect or v.entry == "exact":
        return BIG_CAP, 4
    L = _lib.lib()
    return int(L.dmlp_screen_x1_cap_kt(KT, v.kmax)), int(L.dmlp_screen_x1_group_rows_kt(KT, v.kmax))


@dataclass
class Case:
    name: str
    family: str
    variant: str
    prob: Problem
    S: int
    cap: int
    grows: int
    tps: int
    nq: int
    qidx: np.ndarray | None      # rows of the listed queries (None: row p)
    k: np.ndarray                # [Q]
    kmax: int
    kstride: int
    ids: np.ndarray              # [nq, S, cap] int32
    cnt: np.ndarray              # [nq, S] int32
    h: np.ndarray                # [nq, S, 2] fp32
    labels: str | None           # a label space of result_contract, None: no vote
    aimed: tuple = ()
    i32: bool = False            # the pair kernel's lossless int32 rows
    hq: np.ndarray | None = None  # the threshold in force per listed query (builder's record)

    v = property(lambda self: VARIANTS[self.variant])
    rows = property(lambda self: np.arange(self.nq) if self.qidx is None else self.qidx)

    def label_space(self):
        return RC.label_space(self.labels, self.prob.N) if self.labels else (None, 0, 0)


@dataclass
class Result:
    status: np.ndarray     # [nq]
    d: np.ndarray          # [nq, kstride]; slots [0, k) of a handed-back query are not defined
    i: np.ndarray
    label: np.ndarray | None
    cs: np.ndarray | None
    nsurv: np.ndarray      # survivors (-1: overflowed slice)
    surv: list = field(default_factory=list)   # the surviving rows per listed query (None: -1)

    def differs(self, o: "Result", k) -> bool:
        if (self.status != o.status).any():
            return True
        ok = self.status == 0
        return bool((self.i[ok] != o.i[ok]).any() or (self.d[ok] != o.d[ok]).any())


def refine_ref(case: Case, rule: Rule = RULE, capacity: int | None = None) -> Result:
    """What the refine must write for the case (capacity: the member slots of the kernel that
    ran, where that is not the variant's own)."""
    pr, v = case.prob, case.v
    if capacity is not None:
        v = replace(v, capacity=capacity)
    nq, ks = case.nq, case.kstride
    st = np.zeros(nq, np.int32)
    d = np.full((nq, ks), np.inf)
    i = np.full((nq, ks), -1, np.int32)
    nsurv = np.zeros(nq, np.int64)
    surv = []
    for p, q in enumerate(case.rows):
        kq = int(case.k[q])
        if v.entry == "refine":
            if (case.cnt[p] < 0).any():
                rows = None
            else:
                n = [case.cap if rule.to_cap else int(c) for c in case.cnt[p]]
                rows = np.concatenate([case.ids[p, s, :n[s]] for s in range(case.S)]).astype(np.int64)
        else:
            rows, _ = survivors(case.ids[p].view(np.uint32), case.cnt[p], case.h[p], kq, pr.N,
                                case.tps, case.grows, v.collect,
                                pr.score[q] if v.image else None, rule)
        surv.append(rows)
        if rows is None or (v.capacity is not None and len(rows) > v.capacity + rule.cap_delta):
            st[p] = 1
            nsurv[p] = -1 if rows is None else len(rows)
            continue
        nsurv[p] = len(rows)
        d[p], i[p] = rank(pr.Qx[q], pr.X, rows, kq, ks, rule)
    lab = cs = None
    if case.labels:
        labels = case.label_space()[0]
        if i.max() >= len(labels):     # (mutants only) padding rows
            labels = np.concatenate([labels, np.zeros(i.max() + 1 - len(labels), np.int32)])
        lab, cs = RC.finalize_ref(i, case.k[case.rows], labels)
    return Result(st, d, i, lab, cs, nsurv, surv)


# ------------------------------------------------------------------ the builder
class Builder:
    def __init__(self, name, family, variant, prob, S=1, nq=None, qidx=None, k=None, labels="ten",
                 aimed=(), i32=False, cap=None, kstride=None, tps=None, kmax=None):
        v = VARIANTS[variant]
        if kmax is not None:
            v = replace(v, kmax=kmax)
        self.name, self.family, self.variant, self.prob, self.S = name, family, variant, prob, S
        lcap, self.grows = layout(variant, prob.KT) if v.entry != "refine" else (cap, 0)
        self.cap = lcap if cap is None else cap
        self.qidx = None if qidx is None else np.asarray(qidx, np.int32)
        self.nq = len(self.qidx) if qidx is not None else (prob.Q if nq is None else nq)
        self.k = np.full(prob.Q, v.kmax, np.int32) if k is None else np.asarray(k, np.int32).copy()
        self.kmax = v.kmax
        self.kstride = v.kmax + 5 if kstride is None else kstride
        self.labels = labels if v.entry != "exact" else None
        self.aimed, self.i32 = tuple(aimed), i32
        self.g = Groups(prob, S, self.grows, tps) if self.grows else None
        self.tps = self.g.tps if self.g else X1.tiles_per_slice((prob.N + 63) // 64, S)
        self.ids = np.zeros((self.nq, S, self.cap), np.int32)
        self.cnt = np.zeros((self.nq, S), np.int32)
        self.h = np.zeros((self.nq, S, 2), np.float32)
        self.h[:, :, 0] = -np.inf
        for p in range(self.nq):
            self.h[p, :, 1] = prob.eps[self.row(p)]
        self.listed = {}

    def row(self, p):
        return p if self.qidx is None else int(self.qidx[p])

    def put(self, p, s, groups, thr=None, eps=None, keys=None, overflow=False):
        """the entries of (query p, slice s) in this order; keys: stated keys (default: the
        ordered 16-bit key of the group's fp32 score maximum)"""
        groups = np.asarray(groups, np.int64).reshape(-1)
        assert len(np.unique(groups)) == len(groups) <= self.cap, "distinct entries within cap"
        if self.g is not None:
            assert (groups < len(self.g.rows[s])).all(), "group index outside the slice"
            assert (self.g.n_real(s)[groups] > 0).all(), "a group of padding rows"
            if keys is None:
                keys = X1.key16(self.g.gmax[s][self.row(p), groups])
            self.ids[p, s, :len(groups)] = ((np.asarray(keys, np.int64) << 16) | groups
                                            ).astype(np.uint32).view(np.int32)
        else:
            self.ids[p, s, :len(groups)] = groups
        self.cnt[p, s] = -1 if overflow else len(groups)
        self.listed[p, s] = groups
        if thr is not None:
            self.h[p, s, 0] = thr
        if eps is not None:
            self.h[p, s, 1] = eps

    def _garbage(self):
        pr = self.prob
        for p in range(self.nq):
            q = self.row(p)
            for s in range(self.S):
                n = max(int(self.cnt[p, s]), 0)
                free = self.cap - n
                if free == 0:
                    continue
                mine = self.listed.get((p, s), ()) if self.cnt[p, s] >= 0 else ()
                if self.g is None:    # plain ids: the nearest rows that are not listed anywhere
                    every = np.concatenate([self.listed.get((p, t), np.zeros(0, np.int64))
                                            for t in range(self.S)])
                    near = np.argsort(-pr.score[q], kind="stable")
                    fill = near[~np.isin(near, every)][s::self.S]
                    ent = fill.astype(np.int64)
                else:
                    fill = self.g.best(q, s, full=False, exclude=mine)
                    ent = (0xFFFF << 16) | fill.astype(np.int64)
                if len(ent) == 0:     # an empty slice: its group 0 lies past n_points
                    ent = np.array([0xFFFF << 16 if self.g is not None else 0], np.int64)
                ent = np.resize(ent, free)
                self.ids[p, s, n:] = ent.astype(np.uint32).view(np.int32)

    def clear(self, p):
        """(hq, None) of listed query p, or (hq, slice) of a member within the margin of hq"""
        v = VARIANTS[self.variant]
        if (self.cnt[p] < 0).any():
            return np.float32(-np.inf), None
        q = self.row(p)
        _, hq = survivors(self.ids[p].view(np.uint32), self.cnt[p], self.h[p], int(self.k[q]),
                          self.prob.N, self.tps, self.grows, v.collect,
                          self.prob.score[q] if v.image else None)
        if not v.image or hq == -np.inf:
            return hq, None
        for s in range(self.S):
            rows = self.g.rows[s][self.listed.get((p, s), np.zeros(0, np.int64))].reshape(-1)
            rows = rows[rows < self.prob.N]
            gap = np.abs(self.prob.score[q, rows] - np.float64(hq))
            if not (gap > MARGIN * float(self.prob.eps[q])).all():
                return hq, s
        return hq, None

    def done(self) -> Case:
        self._garbage()
        v = replace(VARIANTS[self.variant], kmax=self.kmax)
        case = Case(self.name, self.family, self.variant, self.prob, self.S, self.cap, self.grows,
                    self.tps, self.nq, self.qidx, self.k, self.kmax, self.kstride, self.ids,
                    self.cnt, self.h, self.labels, self.aimed, self.i32)
        assert (self.k[case.rows] <= v.kmax).all() and (self.k >= 0).all()
        assert 1 <= self.S <= S_MAX and self.kstride >= v.kmax
        case.hq = np.full(self.nq, -np.inf, np.float32)
        if v.entry == "refine":
            for p in range(self.nq):
                every = np.concatenate([self.ids[p, s, :max(self.cnt[p, s], 0)]
                                        for s in range(self.S)])
                assert len(np.unique(every)) == len(every), "duplicate ids"
            return case
        for p in range(self.nq):
            case.hq[p], bad = self.clear(p)
            assert bad is None, f"{self.name}: query {self.row(p)} slice {bad}: a member within eps of the threshold"
        return case


def gap_threshold(scores, eps, T: int):
    """fp32 threshold in the middle of the gap below the T-th largest score, or None when that gap
    is not wider than 2 MARGIN eps (T = 0: above every score)."""
    s = np.sort(np.asarray(scores, np.float64))[::-1]
    m = 2.0 * MARGIN * float(eps) * 1.001
    if T == 0:
        return np.float32(s[0] + 2.0 * m)
    if T >= len(s):
        return np.float32(s[-1] - 2.0 * m)
    if s[T - 1] - s[T] <= m:
        return None
    return np.float32(0.5 * (s[T - 1] + s[T]))


# ------------------------------------------------------------------ case families
N_ONE, N_MOST = 1001, 1011   # the last group holds one real row / all but one (4- and 8-row)


def _scores(b: Builder, p, s, groups):
    rows = b.g.rows[s][np.asarray(groups, np.int64)].reshape(-1)
    return b.prob.score[b.row(p), rows[rows < b.prob.N]]


def _put_at(b: Builder, p, T, n_groups, seed=0, must=(), s=0):
    """n_groups random groups of slice s (the groups of `must` among them) and a threshold below
    the T-th largest of their members' scores, clear of every member by the margin"""
    rng = np.random.default_rng(seed + 7919 * p)
    ng = len(b.g.rows[s])
    pool = np.setdiff1d(np.nonzero(b.g.n_real(s) > 0)[0], must)
    for _ in range(400):
        groups = np.concatenate([rng.permutation(pool)[:n_groups - len(must)],
                                 np.asarray(must, np.int64)])
        thr = gap_threshold(_scores(b, p, s, groups), b.prob.eps[b.row(p)], T)
        if thr is not None and len(_scores(b, p, s, groups)) > T:
            b.put(p, s, groups, thr=thr)
            return groups, thr
    raise AssertionError(f"{b.name}: no clear gap below member {T} of {n_groups} groups of {ng}")


def _capacity_groups(b: Builder, p, T, s=0):
    """full groups of the query's best, then (T not a multiple of the group) a last group cut by
    n_points: T real members in all"""
    g = b.grows
    cutg = [b.g.with_real(s, T % g)] if T % g else []
    return np.concatenate([b.g.best(b.row(p), s, T // g, exclude=cutg), np.array(cutg, np.int64)])


def family_a():
    """Capacity: S = 1, threshold -inf, every listed member survives; survivors at the member
    slots (ranked), one past them (handed back) and one short of them."""
    out = []
    for variant, A in (("pair", 32), ("pair", 40), ("rm64", 32), ("groups", 32), ("groups16", 32),
                       ("groups2", 40), ("collect", 32), ("exact", 32)):
        C = VARIANTS[variant].capacity
        for N, targets, aimed in ((N_ONE, (C, C + 1), ("cap_minus", "cap_plus", "to_cap", "swap_grows")),
                                  (N_MOST, (C - 1, C), ("cap_minus", "to_cap", "swap_grows"))):
            kind = "uni" if VARIANTS[variant].image else "plain"
            b = Builder(f"A-{variant}-A{A}-N{N}", "A", variant, problem(kind, A, N), nq=5,
                        aimed=aimed)
            for p in range(b.nq):
                b.put(p, 0, _capacity_groups(b, p, targets[p % 2]))
            out.append(b.done())
    return out


def _tie_groups(b: Builder, n):
    return b.g.of_rows(0, np.arange(TIE0, TIE1))[:n]


def family_b():
    """Order: identical rows (ids descending), near-tied rows (the order of summation), true
    neighbours past candidate position 64 (the pre-filter's bound comes from the first 64), every
    member at one distance, real rows at distance +inf before the padding."""
    out = []
    for variant, A in (("pair", 32), ("groups", 32), ("groups2", 40), ("collect", 32),
                       ("exact", 32)):
        v = VARIANTS[variant]
        b = Builder(f"B-ties-{variant}", "B", variant, problem("uni" if v.image else "plain", A, N_ONE),
                    nq=2, aimed=("id_asc", "to_cap"))
        g = b.grows
        b.k[0] = 16
        b.put(0, 0, np.concatenate([b.g.best(0, 0, 2, exclude=_tie_groups(b, 128)),
                                    _tie_groups(b, 32 // g)[::-1]]))
        b.k[1] = v.kmax                       # every member at one distance
        b.put(1, 0, _tie_groups(b, min(v.capacity, TIE1 - TIE0) // g))
        out.append(b.done())
    for variant, A in (("pair", 5), ("pair", 32), ("groups", 5), ("groups", 32), ("collect", 32),
                       ("exact", 5)):
        v = VARIANTS[variant]
        pr = problem("near", A)
        b = Builder(f"B-near-{variant}-A{A}", "B", variant, pr, nq=1, aimed=("r2l",))
        block = np.arange(1000, 1000 + NEAR_P)
        inside = [g for g in b.g.of_rows(0, block) if np.isin(b.g.rows[0][g], block).all()]
        b.put(0, 0, inside[:min(v.capacity, 96) // b.grows])
        out.append(b.done())
    for variant, A in (("groups", 32), ("groups2", 40), ("rm64", 32)):
        pr = problem("uni", A, N_ONE)
        b = Builder(f"B-prefilter-{variant}", "B", variant, pr, qidx=[9, 4, 2, 30], aimed=("to_cap",))
        for p in range(b.nq):
            q, g = b.row(p), b.grows
            kq = 6 if g == 8 else 12
            b.k[q] = kq
            near_rows = RC.topk_ref(RC.dist_l2r(pr.Qx[q], pr.X), kq)[1]
            near = b.g.of_rows(0, near_rows)
            far = b.g.best(q, 0, exclude=near)[::-1][:64 // g + 1]
            assert len(far) * g >= 64 and (len(far) + len(near)) * g <= GROUP_MEMBERS
            b.put(p, 0, np.concatenate([far, near]))
        out.append(b.done())
    for variant, cap in (("exact", None), ("refine", 128)):
        pr = problem("plain", 9, N_ONE)
        b = Builder(f"B-inf-{variant}", "B", variant, pr, qidx=[3, 11], cap=cap, aimed=("to_cap",))
        inf_rows = np.array([7, pr.N // 2, pr.N - 2])
        for p in range(b.nq):
            b.k[b.row(p)] = 64
            if variant == "exact":
                b.put(p, 0, np.concatenate([b.g.of_rows(0, inf_rows), b.g.best(b.row(p), 0, 1)]))
            else:
                b.put(p, 0, np.concatenate([inf_rows, np.arange(400, 410)]))
        out.append(b.done())
    return out


def family_c(hl: int = 1):
    """The threshold decides (S = 1): fewer than k survive; the survivors are at the member slots,
    and one past them, while the listed members are well past both; a listed group's key lies
    below key16(hq)."""
    out = []
    for variant, A in ((("pair", 32), ("pair", 40), ("groups", 32), ("groups2", 40), ("collect", 32))
                       if hl == 1 else (("groups", 32), ("groups2", 40))):
        v = VARIANTS[variant]
        b = Builder(f"C-{variant}-A{A}" + ("-bf16" if hl == 2 else ""), "C", variant,
                    problem("uni", A, N_ONE, hl), qidx=[5, 9, 2, 12, 40],
                    aimed=("no_threshold", "cap_minus", "cap_plus", "to_cap"))
        C, g = v.capacity, b.grows
        many = min(b.cap - 4, 2 * C // g - 2) if C < BIG_MEMBERS else C // g + 12
        if hl == 2:    # bf16: eps is 8 times fp16's, clear gaps are found in the sparse tail only
            many = C // g + 2
        b.k[5] = 16
        _put_at(b, 0, 5, 4)
        _put_at(b, 1, C, many)
        _put_at(b, 2, C + 1, many)
        worst = b.g.best(b.row(3), 0)[-1:]
        _, thr = _put_at(b, 3, 3, 5, must=worst)
        key_w = X1.key16(b.g.gmax[0][b.row(3), worst])[0]
        assert key_w < X1.key16(np.array([thr], np.float32))[0], "the worst group's key must be dead"
        b.k[40] = 7
        _put_at(b, 4, 10, 6)
        out.append(b.done())
    return out


def _global_case(name, variant, A, S, ks, per_slice, seed, aimed, hl=1, kind=None):
    """per_slice best groups of every slice that has any (rotated by the seed); the thresholds in
    cand_h are +inf where the rule must not read them (S > 1, not collect)"""
    v = VARIANTS[variant]
    kind = kind or ("uni" if v.image else "plain")
    b = Builder(name, "D", variant, problem(kind, A, N_ONE, hl) if kind != "plain" else problem(kind, A, N_ONE),
                S=S, qidx=list(range(3, 3 + len(ks))), aimed=aimed)
    for p, kq0 in enumerate(ks):
        q = b.row(p)
        for attempt in range(60):
            rng = np.random.default_rng(1000 * seed + 60 * p + attempt)
            kq, M = kq0, 0
            for s in range(S):
                if len(b.g.rows[s]) == 0:
                    b.put(p, s, [], thr=np.inf)
                    continue
                best = b.g.best(q, s, full=False)
                take = best[np.sort(rng.permutation(min(len(best), per_slice + 4))[:per_slice])]
                tie = np.arange(TIE0, TIE1)
                tie = tie[(tie >= s * b.tps * 64) & (tie < (s + 1) * b.tps * 64)]
                if kq == "dup" and len(tie):   # groups of identical rows: identical keys
                    tg = b.g.of_rows(s, tie)[:per_slice - 1]
                    take = np.concatenate([take[~np.isin(take, tg)][:1], tg])
                b.put(p, s, take, thr=np.inf if not v.collect else -1e30)
                M += len(take)
            keys = np.sort(np.concatenate([b.ids[p, s, :b.cnt[p, s]].view(np.uint32) >> 16
                                           for s in range(S)]).astype(np.int64))[::-1]
            if kq == "M":
                kq = M
            elif kq == "M+":
                kq = M + 2
            elif kq == "dup":  # the k-th and the (k + 1)-th largest key equal, a larger one above
                dup = [j for j in range(2, min(len(keys), v.kmax)) if keys[j - 1] == keys[j]
                       and keys[0] > keys[j]]
                assert dup, f"{name}: no duplicated key at a rank boundary"
                kq = dup[0]
            assert kq <= v.kmax, (name, kq)
            b.k[q] = kq
            if b.clear(p)[1] is None:
                break
        else:
            raise AssertionError(f"{name}: query {q}: no selection clear of the threshold")
    return b.done()


def _first_clear(make, n=40):
    for seed in range(n):
        try:
            return make(seed)
        except AssertionError as e:
            if "within eps" not in str(e):
                raise
    raise AssertionError("no seed keeps every member clear of the threshold")


def family_d():
    """Global threshold: S in {2, 4}, a short last and an empty slice (S = 7 over 16 tiles), S = 256;
    k-th key duplicated at the rank boundary; M == k and M < k; per-slice eps with the maximum in
    a middle slice; collect seeds above and below the k-th key."""
    out = []
    ks = (4, 16, "M", "M+", "dup")
    for variant, A in (("groups", 32), ("groups2", 40), ("collect", 32), ("exact", 32)):
        for S, per in ((2, 6), (4, 4), (7, 3), (256, 2)):
            if variant in ("groups2", "exact") and S in (2, 7):
                continue
            aimed = ("to_cap",)
            out.append(_first_clear(lambda seed: _global_case(
                f"D-{variant}-S{S}", variant, A, S, ks, per, seed, aimed)))
    # per-slice eps, the largest in a middle slice: the survivors straddle the member slots
    for variant, A in (("groups", 32), ("groups2", 40)):
        def make(seed, variant=variant, A=A):
            b = Builder(f"D-eps-{variant}", "D", variant, problem("uni", A, N_ONE), S=4,
                        qidx=[6, 21], aimed=("eps_slice0", "no_2eps"))
            C = VARIANTS[variant].capacity
            per = 2 * C // b.grows // 4
            for p in range(b.nq):
                q = b.row(p)
                b.k[q] = 8
                sc = []
                for s in range(4):
                    take = np.roll(b.g.best(q, s, full=False)[:per + 3], -(seed % 3))[:per]
                    b.put(p, s, take, thr=np.inf)
                    sc.append(_scores(b, p, s, take))
                sc = np.sort(np.concatenate(sc))[::-1]
                keys = np.sort(np.concatenate([b.ids[p, s, :per].view(np.uint32) >> 16
                                               for s in range(4)]).astype(np.int64))[::-1]
                t = float(X1.decode16(keys[7]))
                eps0 = float(b.prob.eps[q])
                assert (sc >= t - 2 * eps0).sum() <= C - 8
                # the largest eps puts the threshold into a clear gap past the member slots
                T = next(T for T in range(C + 4 + 8 * p, len(sc))
                         if gap_threshold(sc, eps0, T) is not None)
                b.h[p, 2, 1] = np.float32((t - float(gap_threshold(sc, eps0, T))) / 2.0)
                assert b.h[p, 2, 1] > b.h[p, 0, 1]
            return b.done()
        out.append(_first_clear(make))
    # the k-th key duplicated at the rank boundary: counted without multiplicity the threshold
    # falls and the survivors pass the member slots
    for variant, A in (("groups", 32), ("groups2", 40)):
        pr = problem("uni", A, N_ONE)
        # queries 0 and 1 lie on the identical rows: their groups hold the largest keys
        b = Builder(f"D-dup-{variant}", "D", variant, pr, S=4, qidx=[1, 0], aimed=("kth_distinct",))
        C, g = VARIANTS[variant].capacity, b.grows
        every_tie = _tie_groups(b, C)
        ties = every_tie[:(C - 8) // g]
        for p in range(b.nq):
            q = b.row(p)
            key = lambda s, grp: X1.key16(b.g.gmax[s][q, grp])
            tie_key = key(0, ties[:1])[0]
            b.k[q] = len(ties) - 1 - p
            b.put(p, 0, ties, thr=np.inf)
            for attempt in range(60):
                rng = np.random.default_rng(60 * p + attempt)
                for s in range(1, 4):
                    low = b.g.best(q, s, full=False)
                    low = low[key(s, low) < tie_key]
                    b.put(p, s, low[np.sort(rng.permutation(16)[:12])], thr=np.inf)
                one = Case(b.name, "D", variant, b.prob, 4, b.cap, g, b.tps, 1, b.qidx[p:p + 1], b.k,
                           b.kmax, b.kstride, b.ids[p:p + 1], b.cnt[p:p + 1], b.h[p:p + 1], None)
                if (b.clear(p)[1] is None and refine_ref(one).status[0] == 0
                        and refine_ref(one, MUTANTS["kth_distinct"]).status[0] == 1):
                    break
            else:
                raise AssertionError(f"{b.name}: query {q}: no selection straddles the member slots")
        out.append(b.done())
    # collect: the seed above the k-th key's threshold, and below it
    b = Builder("D-collect-seed", "D", "collect", problem("uni", 32, N_ONE), S=2,
                qidx=[8, 13, 17], aimed=("no_threshold", "to_cap"))
    for p in range(b.nq):
        q = b.row(p)
        b.k[q] = 12
        for attempt in range(60):
            rng = np.random.default_rng(60 * p + attempt)
            sc = []
            for s in range(2):
                take = b.g.best(q, s)[np.sort(rng.permutation(26)[:20])]
                b.put(p, s, take)
                sc.append(_scores(b, p, s, take))
            above = gap_threshold(np.concatenate(sc), b.prob.eps[q], 9 + p)
            b.h[p, :, 0] = above if p < 2 and above is not None else np.float32(-1e30)
            if (p == 2 or above is not None) and b.clear(p)[1] is None:
                break
        else:
            raise AssertionError("D-collect-seed: no selection clear of the threshold")
    case = b.done()
    assert (case.hq[:2] == case.h[:2, 0, 0]).all() and case.hq[2] > case.h[2, 0, 0]
    out.append(case)
    return out


GEOMETRY_NQ = (1, 2, 7, 8, 9, 70)


def family_e():
    """Geometry: nq around the kernels' queries per workgroup, qidx null and an unsorted strict
    subset, k_q in {0, 1, survivors, survivors + 3, kmax}, kstride = kmax + 5, a pair-kernel wave
    with 0 and 64 survivors, an overflowed slice beside a good one, labels given and null, label
    spaces inside the LDS histogram and without a range."""
    out = []
    for variant, A in (("pair", 32), ("pair", 40), ("groups", 32), ("groups2", 40), ("collect", 32),
                       ("exact", 32)):
        v = VARIANTS[variant]
        pr = problem("uni" if v.image else "plain", A, N_ONE)
        for nq in GEOMETRY_NQ:
            if variant in ("collect", "exact", "groups2") and nq not in (7, 9):
                continue
            qidx = None if nq in (1, 8, 70) else np.random.default_rng(nq).permutation(pr.Q)[:nq]
            labels = "ten" if nq % 2 == 0 else "unknown"
            if variant != "pair" and nq == 9:
                labels = None
            b = Builder(f"E-{variant}-A{A}-nq{nq}", "E", variant, pr, nq=nq, qidx=qidx,
                        labels=labels, aimed=("no_cut", "to_cap") if nq > 1 else ("to_cap",))
            g = b.grows
            for p in range(b.nq):
                q, pat = b.row(p), (p + nq) % 8
                if pat == 0:                                   # nothing listed
                    b.put(p, 0, [])
                elif pat == 1:                                 # the member slots full
                    b.put(p, 0, _capacity_groups(b, p, v.capacity))
                elif pat == 2:                                 # an overflowed slice
                    b.put(p, 0, b.g.best(q, 0, 3), overflow=True)
                elif pat == 3:                                 # a cut group, k past the survivors
                    b.put(p, 0, _capacity_groups(b, p, 2 * g + 1))
                    b.k[q] = 2 * g + 1 + 3
                elif pat == 4:
                    b.put(p, 0, b.g.best(q, 0, 3))
                    b.k[q] = 0
                elif pat == 5:
                    b.put(p, 0, b.g.best(q, 0, 3)[::-1])
                    b.k[q] = 1
                elif pat == 6:
                    b.put(p, 0, b.g.best(q, 0, 2))
                    b.k[q] = 2 * g
                else:
                    b.put(p, 0, b.g.best(q, 0, 5))
            out.append(b.done())
    return out


PAIR_A = (5, 30, 31, 32, 33, 40, 62, 63, 64)


def family_f():
    """Row forms of the pair kernel: fp64 rows and lossless int32 rows at every load branch (int4,
    double2, scalar) and a partial last 32-attribute chunk."""
    out = []
    for A in PAIR_A:
        for i32 in (False, True):
            pr = problem("uni", A, 333)
            b = Builder(f"F-pair-A{A}-{'i32' if i32 else 'f64'}", "F", "pair", pr, nq=9, i32=i32,
                        aimed=("to_cap",))
            for p in range(b.nq):
                b.put(p, 0, b.g.best(p, 0, 1 + p % 8, full=False))
                b.k[p] = (32, 1, 17, 8)[p % 4]
            out.append(b.done())
    return out


def family_g():
    """Plain id lists (dmlp_refine): M <= 64; M in 65..P with k <= 64 and with k in 65..128; M > P
    (the running top-k, re-sorted several times); k = 256 at cap 512; an overflowed slice; rows at
    distance +inf; ids of nearer rows past the counts."""
    out = []
    for cap in (128, 256, 512):
        for S in (1, 4):
            for A in ((9,) if (cap, S) != (128, 4) else (9, 8)):
                pr = problem("plain", A, N_ONE)
                kmax = 256 if cap == 512 else 128
                b = Builder(f"G-refine-cap{cap}-S{S}-A{A}", "G", "refine", pr, S=S, cap=cap, nq=8,
                            kmax=kmax, aimed=("to_cap", "id_asc"))
                rng = np.random.default_rng(cap + S)
                P = 512 if cap > 256 else 256
                plan = [(40, 16), (100, 30), (min(S * cap, P) - 3, min(100, kmax)),
                        (min(S * cap - 9, 900), kmax), (120, kmax), (70, 64), (20, 25), (65, 0)]
                for p, (M, kq) in enumerate(plan):
                    b.k[p] = kq
                    rows = rng.permutation(pr.N)[:M]
                    if p == 0:    # the identical rows, on their query
                        rows = np.concatenate([np.arange(TIE0 + 3, TIE0 + 33), rows[rows < TIE0][:10]])
                    if p == 6:    # rows at distance +inf, k past the finite ones
                        rows = np.concatenate([[7, pr.N // 2, pr.N - 2], np.arange(300, 317)])
                    parts = np.array_split(rows, S)
                    for s in range(S):
                        b.put(p, s, parts[s], overflow=(p == 5 and s == S - 1))
                out.append(b.done())
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case of every family on the host-rendered fp16 image (and the image-free forms)"""
    every = family_a() + family_b() + family_c() + family_d() + family_e() + family_f() + family_g()
    named = {c.name: c for c in every}
    assert len(named) == len(every)
    return named
