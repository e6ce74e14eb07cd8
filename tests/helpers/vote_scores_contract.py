"""Reference of the class-score contract (dmlp.h: dmlp_vote_scores / dmlp_cpu_vote_scores) in plain
Python, and the lists the contract tests feed it.  Nothing here calls libdmlp: counts are Python
integers, a score is accumulated one np.float64 add at a time in list order with np.float64(1.0) /
d, the winner is the max of (score, count, label) tuples.  tests/test_vote_scores_model.py pins it
against the CPU twin, dmlp_cpu_finalize and the vote curve; tests/test_vote_scores.py compares the
kernel with it slot for slot, scores on their bits.

  read    slots [0, min(k_q, kstride)) of a row — no 256-slot clamp
  kept    id >= 0, id != skip_q, label in [label_lo, label_lo + nclass); in list order
  count   kept entries per class
  score   mode 0: float(count); mode 1: the sum of w_e left to right from 0.0, w_e = 1 / d_e, or
          (d_e == 0 ? 1 : 0) when a kept entry of the row has d == 0
  label   the class with count > 0 and the largest (score, count, label); -1 for an empty row

The lists are vote_curve_contract.make_lists' (alternating / staircase / equal / tail padding / +inf
tail / negative id in the middle, five skips, six k choices; distances are sorted small integers
from 0, so most rows take the zero-distance rule), followed by SPECIAL rows with strictly positive
distances (special_rows)."""
from __future__ import annotations

import functools

import numpy as np

import result_contract as RC
import vote_curve_contract as VC

CMAX = 4096          # dmlp_vote_scores_cmax()
CHUNK = 256          # slots the kernel compacts at a time
N_IDS = VC.N_IDS
TINY = 2.0 ** -53    # 1 / TINY = 2^53: the next double is 2^53 + 2
SUB = 1e-310         # subnormal, 1 / SUB overflows to +inf
SUB_MIN = 5e-324     # the smallest subnormal
HUGE = 1.7e308       # 1 / HUGE is subnormal


def scores_ref(ids, k, labels, label_lo, nclass, mode, dist=None, skip=None, r2l=False):
    """(count [Q, nclass] int32, score [Q, nclass] float64, label [Q] int32).  r2l sums a class's
    weights from the last entry down: a wrong order, for the model test."""
    ids = np.asarray(ids)
    Q, ks = ids.shape
    count = np.zeros((Q, nclass), np.int32)
    score = np.zeros((Q, nclass), np.float64)
    label = np.full(Q, -1, np.int32)
    one = np.float64(1.0)
    for q in range(Q):
        n = max(0, min(int(k[q]), ks))
        kept = []
        for e in range(n):
            i = int(ids[q, e])
            if i < 0 or (skip is not None and i == int(skip[q])):
                continue
            c = int(labels[i]) - label_lo
            if 0 <= c < nclass:
                kept.append((c, np.float64(dist[q, e]) if mode == 1 else None))
        cnt = [0] * nclass
        for c, _ in kept:
            cnt[c] += 1
        if mode == 1:
            zero = any(d == 0 for _, d in kept)
            s = [np.float64(0.0)] * nclass
            with np.errstate(divide="ignore", over="ignore"):
                for c, d in (reversed(kept) if r2l else kept):
                    w = (one if d == 0 else np.float64(0.0)) if zero else one / d
                    s[c] = s[c] + w
        else:
            s = [np.float64(c) for c in cnt]
        count[q] = cnt
        score[q] = s
        cand = [(s[c], cnt[c], label_lo + c) for c in range(nclass) if cnt[c] > 0]
        if cand:
            label[q] = max(cand)[2]
    return count, score, label


# ------------------------------------------------------------------ labels
def remap_ten(labels, label_lo, nclass):
    """The ten labels 0..9 of the "ten" space mapped into and around [label_lo, label_lo + nclass):
    both ends, the middle, the classes on both sides of a 64-lane pass, and one label below and
    one above the range (their entries are dropped)."""
    last = nclass - 1
    cand = [0, last, nclass // 2, min(63, last), min(64, last), min(65, last), min(1, last),
            max(last - 1, 0), -1, nclass]
    return (label_lo + np.array(cand, np.int64)[labels]).astype(np.int32)


# ------------------------------------------------------------------ special rows
# (name, distances, roles): a = the largest label of the range that occurs, b = the smallest, c = a
# third class (or x), x = an entry that is dropped (a label outside the range, else id -5).
SPECIAL = (
    # left to right a = (2^53 + 1 -> 2^53) + 1 -> 2^53 and b = 2^53 + 2: b wins on the score; any
    # other order gives a = 2 + 2^53 = b, and a wins on its count of 3
    ("order", (TINY, TINY, 0.5, 1.0, 1.0), "abbaa"),
    ("inf_count", (SUB_MIN, SUB, SUB), "abb"),       # both at +inf: b has more entries
    ("inf_label", (SUB_MIN, SUB), "ba"),             # both at +inf, one entry each: the larger label
    ("huge", (HUGE, HUGE, 1.75e308), "bba"),         # subnormal weights: b = 2 w > a
    ("all_inf", (np.inf,) * 4, "abbx"),              # every score 0: b's count decides
    ("tie", (2.0, 2.0), "ba"),                       # score tie, count tie: the larger label
    ("outside", (0.25, 0.5, 1.0), "xbx"),            # only b is counted
    ("nothing", (0.25, 0.5), "xx"),                  # -1
)


def _role_ids(labels, label_lo, nclass):
    rel = labels.astype(np.int64) - label_lo
    inside = np.flatnonzero((rel >= 0) & (rel < nclass))
    outside = np.flatnonzero((rel < 0) | (rel >= nclass))
    vals = np.unique(labels[inside])
    first = lambda v: int(np.flatnonzero(labels == v)[0])   # noqa: E731
    x = int(outside[0]) if len(outside) else -5
    a, b = first(vals[-1]), first(vals[0])
    c = first(vals[len(vals) // 2]) if len(vals) >= 3 else x
    return {"a": a, "b": b, "c": c, "x": x}


def special_rows(kstride, labels, label_lo, nclass, only=None):
    """(ids, dist, names): every SPECIAL row that fits at slot 0 (padding behind it), and "order"
    again behind class-c filler at distance 3 in the middle of the list, across the boundary of
    the first 256-slot chunk (slots 254 .. 258) and behind 255 DROPPED fillers (the pattern's
    entries are then the only kept ones: one in the first chunk of slots, four in the second).
    `only`: the names of the rows to build, for cases that must stay small."""
    role = _role_ids(labels, label_lo, nclass)
    rows = []
    for name, d, roles in SPECIAL:
        rows.append((name, 0, "c", d, roles))
    _, d, roles = SPECIAL[0]
    rows += [("order_mid", kstride // 2 - 2, "c", d, roles),
             ("order_chunk", CHUNK - 2, "c", d, roles),
             ("order_dropped", CHUNK - 1, "x", d, roles)]
    ids, dist, names = [], [], []
    for name, at, fill, d, roles in rows:
        if at < 0 or at + len(d) > kstride or (only is not None and name not in only):
            continue
        ri = np.full(kstride, -1, np.int32)
        rd = np.full(kstride, np.inf, np.float64)
        ri[:at], rd[:at] = role[fill], 3.0
        ri[at:at + len(d)] = [role[r] for r in roles]
        rd[at:at + len(d)] = d
        ids.append(ri)
        dist.append(rd)
        names.append(name)
    return ids, dist, names


def make_lists(kstride, nq, space="ten", seed=0, nclass=None, label_lo=None, only=None):
    """dict(ids [R, kstride] i32, dist f64, k [R] i32, skip [R] i32, labels [N_IDS] i32, label_lo,
    nclass, mid_negative [R] bool, names {special name: row}): nq rows of
    vote_curve_contract.make_lists, then the special rows (those named in `only` when given; k =
    kstride, skip -1).  With nclass (and label_lo) the "ten" labels are remapped by remap_ten;
    otherwise the space's own range is used (the labels' own when the space states none)."""
    L = VC.make_lists(kstride, kstride, nq, space, seed)
    labels, lo, hi = RC.label_space(space, N_IDS, seed)
    if nclass is not None:
        assert space == "ten"
        labels = remap_ten(labels, label_lo, nclass)
    else:
        if (lo, hi) == (0, 0):
            lo, hi = int(labels.min()), int(labels.max()) + 1
        label_lo, nclass = lo, hi - lo
    si, sd, names = special_rows(kstride, labels, label_lo, nclass, only)
    ns = len(si)
    cat = lambda a, b, dt: np.concatenate([a, np.array(b, dt).reshape(ns, -1)]) if ns else a  # noqa: E731
    return dict(ids=cat(L["ids"], si, np.int32), dist=cat(L["dist"], sd, np.float64),
                k=np.concatenate([L["k"], np.full(ns, kstride, np.int32)]),
                skip=np.concatenate([L["skip"], np.full(ns, -1, np.int32)]),
                mid_negative=np.concatenate([L["mid_negative"], np.zeros(ns, bool)]),
                labels=labels, label_lo=int(label_lo), nclass=int(nclass),
                names={name: nq + j for j, name in enumerate(names)})


@functools.lru_cache(maxsize=None)
def case(kstride, nq, space="ten", seed=0, nclass=None, label_lo=None, mode=1, with_skip=True,
         only=None):
    """(lists, reference) of one case, computed once and shared by the tests that use it; the
    arrays are read-only."""
    L = make_lists(kstride, nq, space, seed, nclass, label_lo, only)
    ref = scores_ref(L["ids"], L["k"], L["labels"], L["label_lo"], L["nclass"], mode, L["dist"],
                     L["skip"] if with_skip else None)
    for a in [v for v in L.values() if isinstance(v, np.ndarray)] + list(ref):
        a.setflags(write=False)
    return L, ref
