"""Reference of the weighted vote-curve contract (dmlp.h: dmlp_vote_curve_weighted /
dmlp_cpu_vote_curve_weighted) in plain Python, and the lists the contract tests feed it.  Nothing
here calls libdmlp: a row is walked entry by entry, a weight is one np.float64 division, a running
score one np.float64 add, a key the Python tuple (score, count, label), and the winner of a prefix
the running max of the keys.  tests/test_weighted_curve_model.py pins it against the CPU twin, the
uniform curve and dmlp_cpu_vote_scores at every prefix; tests/test_weighted_curve.py compares the
kernel with it slot for slot, scores on their bits.

  read      slots [0, min(k_q, kstride, 256)) of a row
  kept      id >= 0 and id != skip_q, in order; m = min(#kept, kcap)
  weight    mode 0: 1; mode 1: the FIRST kept entry decides: at d == 0, w_e = (d_e == 0 ? 1 : 0);
            otherwise w_e = 1 / d_e
  key_e     (s_e, c_e, label_e): score and count of e's class over the kept e' <= e, the score
            summed left to right from 0.0 (mode 0: float(c_e))
  label[j]  j < m: the label of the largest key over the first j + 1 kept entries; j >= m:
            label[m - 1], or -1 (m = 0)
  score[j]  that key's score, repeated alike; 0.0 for m = 0
  lists     the kept entries j < m, then (+inf, -1)
  hits[j]   rows with label[j] == truth_q

The lists are vote_curve_contract.make_lists' (seven recipes, six k choices, five skips; sorted
small-integer distances, from 0 on most rows — every third row is shifted by 1, so that its weights
are 1 / d throughout), followed by SPECIAL rows built from vote_scores_contract's constants."""
from __future__ import annotations

import functools

import numpy as np

import result_contract as RC
import vote_curve_contract as VC
import vote_scores_contract as VS

SLOTS = VC.SLOTS
N_IDS = VC.N_IDS
ORDER_COLUMN = 4     # prefix 5 of the "order" pattern: the column a wrong summation order changes


def _weights(dk, mode):
    one, nil = np.float64(1.0), np.float64(0.0)
    if mode == 0:
        return [one] * len(dk)
    zero = len(dk) > 0 and dk[0] == 0
    with np.errstate(divide="ignore", over="ignore"):
        return [(one if d == 0 else nil) if zero else one / d for d in dk]


def row_ref(lab, dk, mode, r2l=False):
    """([winner label], [winner score]) of every prefix of one row's kept entries (labels lab,
    distances dk).  r2l: each prefix's class scores summed from its last entry down — a wrong
    order, for the model test."""
    w = _weights([np.float64(d) for d in dk], mode)
    out_l, out_s = [], []
    if r2l:
        for j in range(len(lab)):
            s, c = {}, {}
            for e in range(j, -1, -1):
                s[lab[e]] = s.get(lab[e], np.float64(0.0)) + w[e]
                c[lab[e]] = c.get(lab[e], 0) + 1
            best = max((s[v], c[v], v) for v in s)
            out_l.append(best[2])
            out_s.append(best[0])
        return out_l, out_s
    s, c, best = {}, {}, None
    for e, v in enumerate(lab):
        c[v] = c.get(v, 0) + 1
        s[v] = s.get(v, np.float64(0.0)) + w[e] if mode == 1 else np.float64(c[v])
        key = (s[v], c[v], v)
        best = key if best is None else max(best, key)
        out_l.append(best[2])
        out_s.append(best[0])
    return out_l, out_s


def kept_of(ids, k, q, kcap, skip=None):
    ks = ids.shape[1]
    n = max(0, min(int(k[q]), ks, SLOTS))
    return [e for e in range(n)
            if ids[q, e] >= 0 and (skip is None or int(ids[q, e]) != int(skip[q]))][:kcap]


def curve_ref(ids, k, labels, kcap, mode, dist, skip=None, truth=None, r2l=False):
    """(label [Q, kcap] int32, score [Q, kcap] float64, hits int64 [kcap] | None, (dist, ids)
    [Q, kcap])."""
    ids = np.asarray(ids)
    Q = ids.shape[0]
    lab = np.full((Q, kcap), -1, np.int32)
    sc = np.zeros((Q, kcap), np.float64)
    od = np.full((Q, kcap), np.inf, np.float64)
    oi = np.full((Q, kcap), -1, np.int32)
    for q in range(Q):
        kept = kept_of(ids, k, q, kcap, skip)
        m = len(kept)
        if not m:
            continue
        kid = [int(ids[q, e]) for e in kept]
        dk = [dist[q, e] for e in kept]
        ll, ss = row_ref([int(labels[i]) for i in kid], dk, mode, r2l)
        lab[q, :m], sc[q, :m] = ll, ss
        lab[q, m:], sc[q, m:] = ll[-1], ss[-1]
        oi[q, :m], od[q, :m] = kid, dk
    hits = None
    if truth is not None:
        hits = (lab == np.asarray(truth)[:, None]).sum(axis=0).astype(np.int64)
    return lab, sc, hits, (od, oi)


# ------------------------------------------------------------------ special rows
# (name, distances, roles): a = an id of the largest label, b = one of the smallest, c = one of a
# third label (or x), x = a dropped entry (id -5), s = an id that the row's skip names.
SPECIAL = (
    # left to right a = (2^53 + 1 -> 2^53) + 1 -> 2^53 and b = 2^53 + 2: b wins prefix 5 on the
    # score; any other order gives a = 2 + 2^53 = b, and a wins on its count of 3
    ("order", (VS.TINY, VS.TINY, 0.5, 1.0, 1.0), "abbaa"),
    ("subnormal", (VS.SUB_MIN, VS.SUB, VS.SUB), "abb"),    # all +inf: the count, then the label
    ("inf_label", (VS.SUB_MIN, VS.SUB), "ba"),
    ("huge", (VS.HUGE, VS.HUGE, 1.75e308), "bba"),         # subnormal weights: b = 2 w > a
    ("all_inf", (np.inf,) * 4, "abbx"),                    # every score 0: the count decides
    ("tie", (2.0, 2.0), "ba"),                             # score and count tie: the larger label
    ("flip", (1.0,) * 8, "babababa"),                      # the winner changes at every prefix
    ("unsorted", (1.0, 0.0, 2.0), "abb"),                  # 1 / d rule: scores 1, +inf, +inf
    ("nothing", (0.25, 0.5), "xx"),                        # -1, 0.0
    ("skip_zero", (0.0, 1.0, 4.0), "sba"),                 # the first KEPT entry (d = 1) decides: b
)


def _role_ids(labels):
    vals = np.unique(labels)
    first = lambda v: int(np.flatnonzero(labels == v)[0])   # noqa: E731
    a, b = first(vals[-1]), first(vals[0])
    c = first(vals[len(vals) // 2]) if len(vals) >= 3 else -5
    s = next(i for i in range(len(labels)) if i not in (a, b, c))
    return {"a": a, "b": b, "c": c, "x": -5, "s": s}


def special_rows(kstride, labels):
    """(ids, dist, skip, names, order_at): every SPECIAL row that fits at slot 0 (padding behind
    it), and "order" again behind class-c filler at distance 3 in the middle of the list and ending
    at slot 256.  order_at: {name: the slot its pattern starts at} of the order-sensitive rows."""
    role = _role_ids(labels)
    rows = [(name, 0, d, roles) for name, d, roles in SPECIAL]
    _, d, roles = SPECIAL[0]
    rows += [("order_mid", kstride // 2 - 2, d, roles), ("order_end", SLOTS - len(d), d, roles)]
    ids, dist, skip, names, order_at = [], [], [], [], {}
    for name, at, d, roles in rows:
        if at < 0 or at + len(d) > kstride or (name == "order_mid" and at == 0):
            continue
        ri = np.full(kstride, -1, np.int32)
        rd = np.full(kstride, np.inf, np.float64)
        ri[:at], rd[:at] = role["c"], 3.0
        ri[at:at + len(d)] = [role[r] for r in roles]
        rd[at:at + len(d)] = d
        ids.append(ri)
        dist.append(rd)
        skip.append(role["s"] if "s" in roles else -1)
        names.append(name)
        if name.startswith("order"):
            order_at[name] = at if role["c"] >= 0 else 0   # (dropped filler: the pattern leads)
    return ids, dist, skip, names, order_at


def make_lists(kcap, kstride, nq, space, seed=0):
    """dict(ids [R, kstride] i32, dist f64, k [R] i32, skip [R] i32, truth [R] i32, labels [N_IDS]
    i32, mid_negative [R] bool, names {special name: row}, order_at {name: slot}): nq rows of
    vote_curve_contract.make_lists, then the special rows (k = kstride)."""
    L = VC.make_lists(kcap, kstride, nq, space, seed)
    dist = L["dist"].copy()
    dist[1::3] += 1.0
    labels = L["labels"]
    si, sd, ss, names, order_at = special_rows(kstride, labels)
    ns = len(si)
    cat = lambda a, b, dt: np.concatenate([a, np.array(b, dt).reshape(ns, -1)]) if ns else a  # noqa: E731
    a_label = int(labels[_role_ids(labels)["a"]])
    return dict(ids=cat(L["ids"], si, np.int32), dist=cat(dist, sd, np.float64),
                k=np.concatenate([L["k"], np.full(ns, kstride, np.int32)]),
                skip=np.concatenate([L["skip"], np.array(ss, np.int32)]),
                truth=np.concatenate([L["truth"], np.full(ns, a_label, np.int32)]),
                mid_negative=np.concatenate([L["mid_negative"], np.zeros(ns, bool)]),
                labels=labels, names={name: nq + j for j, name in enumerate(names)},
                order_at={name: at for name, at in order_at.items()})


def sorted_rows(L, kcap, with_skip=True):
    """bool [R]: the rows whose kept distances are non-decreasing (dmlp_vote_scores' zero-distance
    rule and the first-kept-entry rule agree there)."""
    out = np.zeros(L["ids"].shape[0], bool)
    for q in range(len(out)):
        dk = [L["dist"][q, e] for e in kept_of(L["ids"], L["k"], q, kcap,
                                               L["skip"] if with_skip else None)]
        out[q] = all(x <= y for x, y in zip(dk, dk[1:]))
    return out


@functools.lru_cache(maxsize=None)
def case(kcap, kstride, nq, space, mode, seed=0, with_skip=True):
    """(lists, reference) of one case, computed once and shared by the tests that use it; the
    arrays are read-only."""
    L = make_lists(kcap, kstride, nq, space, seed)
    ref = curve_ref(L["ids"], L["k"], L["labels"], kcap, mode, L["dist"],
                    L["skip"] if with_skip else None, L["truth"])
    for a in [v for v in L.values() if isinstance(v, np.ndarray)] + [ref[0], ref[1], ref[2], *ref[3]]:
        a.setflags(write=False)
    return L, ref
