"""Reference of the vote-curve contract (dmlp.h: dmlp_vote_curve / dmlp_cpu_vote_curve) in NumPy
and Python integers, and the lists the contract tests feed it.  Nothing here calls libdmlp: the
vote of a prefix is result_contract.vote_ref on that prefix, the compaction and the hit counts are
spelled out.  tests/test_vote_curve_model.py pins it against the CPU twin and dmlp_cpu_finalize,
tests/test_vote_curve.py compares the kernel with it slot for slot.

  read      slots [0, min(k_q, kstride, 256)) of a row
  kept      id >= 0 and id != skip_q, in order; m = min(#kept, kcap)
  label[j]  j < m: the vote over the first j + 1 kept entries; j >= m: label[m - 1], or -1 (m = 0)
  lists     the kept entries j < m, then (+inf, -1)
  hits[j]   rows with label[j] == truth_q
"""
from __future__ import annotations

import functools

import numpy as np

import result_contract as RC

SLOTS = 256          # dmlp_vote_curve_kmax()
N_IDS = 400          # ids the lists draw from (> the 300 slots of the widest rows)

# row recipes (row r of a case uses recipe (r + seed) % 7, k choice (r + seed) % 6, skip choice
# (r + seed) % 5: 7, 6 and 5 are coprime, so 210 consecutive rows meet every combination)
RECIPES = ("random", "alternating", "staircase", "equal", "tail_padding", "inf_tail", "mid_negative")
SKIPS = ("first", "middle", "last", "absent", "minus_one")


def curve_ref(ids, k, labels, kcap, skip=None, truth=None, dist=None):
    """(label [Q, kcap] int32, hits int64 [kcap] | None, (dist, ids) [Q, kcap] | None)."""
    ids = np.asarray(ids)
    Q, ks = ids.shape
    lab = np.empty((Q, kcap), np.int32)
    od = np.full((Q, kcap), np.inf, np.float64)
    oi = np.full((Q, kcap), -1, np.int32)
    for q in range(Q):
        n = max(0, min(int(k[q]), ks, SLOTS))
        kept = [e for e in range(n)
                if ids[q, e] >= 0 and (skip is None or int(ids[q, e]) != int(skip[q]))]
        kept = kept[:kcap]
        m = len(kept)
        kid = [int(ids[q, e]) for e in kept]
        for j in range(m):
            lab[q, j] = RC.vote_ref(kid, j + 1, labels)
        lab[q, m:] = lab[q, m - 1] if m else -1
        oi[q, :m] = kid
        if dist is not None:
            od[q, :m] = [dist[q, e] for e in kept]
    hits = None
    if truth is not None:
        hits = np.array([sum(int(lab[q, j]) == int(truth[q]) for q in range(Q))
                         for j in range(kcap)], np.int64)
    return lab, hits, ((od, oi) if dist is not None else None)


def k_choices(kcap, kstride):
    return (0, 1, kcap - 1, kcap, kcap + 1, kstride + 7)


def _pools(labels, rng):
    """Ids of three label values a < b < c (the most frequent ones; a pool may hold one id, and a
    space of two labels gives a < b = c)."""
    vals, counts = np.unique(labels, return_counts=True)
    top = np.sort(vals[np.argsort(-counts, kind="stable")[:3]])
    top = list(top) + [top[-1]] * (3 - len(top))
    return [rng.permutation(np.flatnonzero(labels == v)) for v in top]


def _cycle(pool, n, start=0):
    return pool[(start + np.arange(n)) % len(pool)]


def make_lists(kcap, kstride, nq, space, seed=0):
    """dict(ids [nq, kstride] i32, dist f64, k [nq] i32, skip [nq] i32, truth [nq] i32, labels
    [N_IDS] i32, mid_negative [nq] bool).  Lists are sorted by distance with ties; ids may repeat
    in the patterned rows (a skip then drops every occurrence)."""
    rng = np.random.default_rng(1000 * kcap + 10 * kstride + nq + 7919 * seed)
    labels, _, _ = RC.label_space(space, N_IDS, seed)
    pa, pb, pc = _pools(labels, rng)
    ids = np.full((nq, kstride), -1, np.int32)
    dist = np.full((nq, kstride), np.inf, np.float64)
    k = np.empty(nq, np.int32)
    skip = np.empty(nq, np.int32)
    mid = np.zeros(nq, bool)
    kc = k_choices(kcap, kstride)
    for r in range(nq):
        recipe = RECIPES[(r + seed) % 7]
        k[r] = kc[(r + seed) % 6]
        n_real = kstride
        e = np.arange(kstride)
        if recipe == "alternating":      # a, b, a, b, ...: a tie at every even prefix, b wins it
            row = np.where(e % 2 == 0, _cycle(pa, kstride), _cycle(pb, kstride))
        elif recipe == "staircase":      # a, b, c, a, b, c, ...: the winner moves at every prefix
            row = np.choose(e % 3, [_cycle(pa, kstride), _cycle(pb, kstride), _cycle(pc, kstride)])
        elif recipe == "equal":
            row = _cycle(pa, kstride, r)
        else:
            row = rng.permutation(N_IDS)[:kstride] if kstride <= N_IDS else \
                rng.integers(0, N_IDS, kstride)
            if recipe == "tail_padding":
                n_real = int(rng.integers(0, kstride + 1))
        ids[r, :n_real] = row[:n_real]
        d = np.sort(rng.integers(0, max(2, kstride // 3), n_real).astype(np.float64))
        if recipe == "inf_tail":         # real neighbours at distance +inf
            d[n_real - (n_real + 2) // 3:] = np.inf
        dist[r, :n_real] = d
        n = max(0, min(int(k[r]), kstride, SLOTS))
        if recipe == "mid_negative" and n >= 3:
            ids[r, n // 2] = -7
            mid[r] = True
        how = SKIPS[(r + seed) % 5]
        if how == "minus_one" or n == 0:
            skip[r] = -1
        elif how == "absent":
            skip[r] = N_IDS + 5 if recipe not in ("random", "tail_padding", "inf_tail") else \
                int(np.setdiff1d(np.arange(N_IDS), ids[r])[0]) if kstride < N_IDS else N_IDS + 5
        else:
            skip[r] = ids[r, {"first": 0, "middle": n // 2, "last": n - 1}[how]]
    # the truth: a label of the list's neighbourhood, so that hits are neither 0 nor nq
    truth = np.empty(nq, np.int32)
    for r in range(nq):
        real = ids[r][ids[r] >= 0]
        truth[r] = labels[real[int(rng.integers(0, min(len(real), 4)))]] if len(real) else -1
    return dict(ids=ids, dist=dist, k=k, skip=skip, truth=truth, labels=labels, mid_negative=mid)


@functools.lru_cache(maxsize=None)
def case(kcap, kstride, nq, space, seed=0, with_skip=True):
    """(lists, reference) of one case, computed once and shared by the tests that use it; the
    arrays are read-only."""
    L = make_lists(kcap, kstride, nq, space, seed)
    ref = curve_ref(L["ids"], L["k"], L["labels"], kcap, L["skip"] if with_skip else None,
                    L["truth"], L["dist"])
    for a in list(L.values()) + [ref[0], ref[1], *ref[2]]:
        a.setflags(write=False)
    return L, ref
