"""Reference of the neighbour-mean contract (dmlp.h: dmlp_neighbor_means / dmlp_neighbor_means_curve
and their dmlp_cpu_ twins) in plain Python, and the lists the contract tests feed it.  Nothing here
calls libdmlp: a row is walked entry by entry in list order, every weight, product, sum and quotient
is one np.float64 operation (taken over the T target columns at once, which rounds each column on
its own).  tests/test_neighbor_means_model.py pins it against the CPU twins;
tests/test_neighbor_means.py compares the kernel with it slot for slot, on the bits.

  read    slots [0, min(k_q, kstride)) of a row; the curve additionally stops at slot 256
  kept    id >= 0 and id != skip_q, in list order; m = their number
  weight  mode 0: 1.  mode 1: d_ref / d_e, d_ref the FIRST kept entry's distance; d_ref == 0:
          (d_e == 0 ? 1 : 0); d_ref == +inf: 1
  sums    sum_t = ((p_1 + p_2) + ...) from 0.0, p_e = w_e * targets[id_e][t] (no multiply in mode
          0); wsum = ((w_1 + w_2) + ...) (mode 0: float(m)); mean_t = sum_t / wsum
  means   (mean [T], wsum, m); m == 0: (NaN, 0.0, 0)
  curve   column j < min(m, kcap): the mean over the first j + 1 kept entries; later columns repeat
          the last computed one; all NaN when m == 0

The lists are vote_curve_contract.make_lists' (its rotation of row recipes — alternating / staircase
/ equal / tail padding / +inf tail / a negative id in the middle —, five skips and six k choices, by
import; every other row's distances are shifted by 1, so that both the zero-distance rule and the
d_ref / d division are met), followed by the SPECIAL rows (special_rows)."""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

import vote_curve_contract as VC

TMAX = 256           # dmlp_neighbor_means_tmax()
SLOTS = 256          # slots the curve reads; the chunk of the kernel's compaction
N_IDS = VC.N_IDS
P53 = 2.0 ** 53

# target values of the special rows: row N_IDS + i of the targets holds VALUES[i] in every column
VALUES = (0.0, P53, 1.0, -P53, -1.0, 3.0, 7.0, 1e308, 5.0)
_V = {v: N_IDS + i for i, v in enumerate(VALUES)}
DROP = -5            # an id that is dropped

# (name, distances, target values).  Equal distances give weights of exactly 1, so such a row
# computes the same sums in both modes.
SPECIAL = (
    # left to right ((2^53 + 1 -> 2^53) + 1 -> 2^53) - 2^53 = 0; right to left 2; pairwise 1
    ("order", (2.0,) * 4, (P53, 1.0, 1.0, -P53)),
    # mode 1: w = 1, fl(1 / 3); fl(w_2 * 3) = 1, so the sum is -1 + 1 = 0.0; fused, the unrounded
    # product 1 - 2^-54 gives -5.55e-17
    ("contract", (1.0, 3.0), (-1.0, 3.0)),
    ("zeros", (0.0, 0.0, 1.0, 2.0), (7.0, 3.0, 1e308, 5.0)),      # w = 1, 1, 0, 0: mean 5
    ("all_inf", (np.inf,) * 3, (1.0, 3.0, 7.0)),                  # w = 1, 1, 1
    ("inf_tail", (2.0, 4.0, np.inf, np.inf), (7.0, 3.0, 1e308, 5.0)),   # w = 1, 0.5, 0, 0
    ("subnormal", (5e-324, 1e-320), (3.0, 7.0)),                  # w_2 = fl(1 / 2024)
    ("huge", (1.7e308, 1.75e308), (3.0, 7.0)),                    # 1 / d would be subnormal
    ("overflow", (2.0,) * 3, (1e308, 1e308, 1e308)),              # the sum reaches +inf: no NaN
    ("nothing", (1.0, 2.0), (None, None)),                        # m == 0
)
ORDER_SENSITIVE = ("order", "order_mid", "order_chunk", "order_dropped")
CONTRACT_SENSITIVE = ("contract",)


def _fma(a, b, c):
    """fl(a * b + c) with one rounding, for finite doubles."""
    return np.float64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def row_ref(ids, dist, k, skip, targets, mode, kcap=None, r2l=False, fused=False):
    """One row: (mean [T], wsum, m, curve [kcap, T] | None).  r2l sums from the last kept entry
    down and fused rounds w * y + sum once: wrong arithmetic, for the model test (mean only)."""
    ks = len(ids)
    T = targets.shape[1]
    n = max(0, min(int(k), ks))
    kept = [e for e in range(n) if ids[e] >= 0 and (skip is None or int(ids[e]) != int(skip))]
    m = len(kept)
    one, zero = np.float64(1.0), np.float64(0.0)
    w = []
    if mode == 1 and m:
        dref = np.float64(dist[kept[0]])
        with np.errstate(invalid="ignore"):
            for e in kept:
                x = np.float64(dist[e])
                if dref == 0:
                    w.append(one if x == 0 else zero)
                elif np.isinf(dref):
                    w.append(one)
                else:
                    w.append(dref / x)
    s = np.zeros(T, np.float64)
    ws = zero
    curve = None if kcap is None else np.full((kcap, T), np.nan, np.float64)
    last = -1
    with np.errstate(over="ignore", invalid="ignore"):
        for j, e in (reversed(list(enumerate(kept))) if r2l else enumerate(kept)):
            y = targets[int(ids[e])]
            if mode == 1:
                if fused:
                    s = np.array([_fma(w[j], y[t], s[t]) for t in range(T)], np.float64)
                else:
                    p = w[j] * y
                    s = s + p
                ws = ws + w[j]
            else:
                s = s + y
                ws = np.float64(j + 1)
            if curve is not None and j < kcap and e < SLOTS:
                curve[j] = s / ws
                last = j
        if mode == 0:
            ws = np.float64(m)
        mean = s / ws if m else np.full(T, np.nan, np.float64)
    if curve is not None and last >= 0:
        curve[last + 1:] = curve[last]
    return mean, (ws if m else zero), m, curve


def means_ref(ids, k, targets, mode, dist=None, skip=None, kcap=None, r2l=False, fused=False):
    """(mean [Q, T], wsum [Q], count [Q] int32, curve [Q, kcap, T] | None) of the lists."""
    ids = np.asarray(ids)
    Q = ids.shape[0]
    T = targets.shape[1]
    mean = np.empty((Q, T), np.float64)
    wsum = np.empty(Q, np.float64)
    count = np.empty(Q, np.int32)
    curve = None if kcap is None else np.empty((Q, kcap, T), np.float64)
    for q in range(Q):
        r = row_ref(ids[q], None if dist is None else dist[q], k[q],
                    None if skip is None else skip[q], targets, mode, kcap, r2l, fused)
        mean[q], wsum[q], count[q] = r[0], r[1], r[2]
        if curve is not None:
            curve[q] = r[3]
    return mean, wsum, count, curve


# ------------------------------------------------------------------ lists
def make_targets(T, seed=0):
    """[N_IDS + len(VALUES), T]: full-mantissa values in (-1000, 1000), then the special rows'."""
    rng = np.random.default_rng(4242 + 31 * T + seed)
    return np.concatenate([rng.uniform(-1000.0, 1000.0, (N_IDS, T)),
                           np.repeat(np.array(VALUES, np.float64)[:, None], T, axis=1)])


def special_rows(kstride, only=None):
    """(ids, dist, names): every SPECIAL row that fits at slot 0 (padding behind it), and "order"
    again behind kept fillers (target 0.0, the pattern's distance) in the middle of the list and
    across the slot-256 boundary (slots 254 .. 257), and behind 255 DROPPED entries (the pattern's
    entries are then the only kept ones: one in the first 256 slots, three behind them)."""
    rows = [(name, 0, None, d, v) for name, d, v in SPECIAL]
    _, d, v = SPECIAL[0]
    rows += [("order_mid", kstride // 2 - 2, _V[0.0], d, v),
             ("order_chunk", SLOTS - 2, _V[0.0], d, v),
             ("order_dropped", SLOTS - 1, DROP, d, v)]
    ids, dist, names = [], [], []
    for name, at, fill, d, v in rows:
        if at < 0 or at + len(d) > kstride or (only is not None and name not in only):
            continue
        ri = np.full(kstride, -1, np.int32)
        rd = np.full(kstride, np.inf, np.float64)
        if at:
            ri[:at], rd[:at] = fill, d[0]
        ri[at:at + len(d)] = [DROP if x is None else _V[x] for x in v]
        rd[at:at + len(d)] = d
        ids.append(ri)
        dist.append(rd)
        names.append(name)
    return ids, dist, names


def make_lists(kcap, kstride, nq, T, seed=0, only=None):
    """dict(ids [R, kstride] i32, dist f64, k [R] i32, skip [R] i32, targets [N, T] f64, names
    {special name: row}): nq rows of vote_curve_contract.make_lists (odd rows' distances + 1), then
    the special rows (k = kstride, skip -1)."""
    L = VC.make_lists(kcap, kstride, nq, "ten", seed)
    dist = L["dist"] + (np.arange(nq) % 2)[:, None]
    si, sd, names = special_rows(kstride, only)
    ns = len(si)
    cat = lambda a, b, dt: np.concatenate([a, np.array(b, dt).reshape(ns, -1)]) if ns else a  # noqa: E731
    return dict(ids=cat(L["ids"], si, np.int32), dist=cat(dist, sd, np.float64),
                k=np.concatenate([L["k"], np.full(ns, kstride, np.int32)]),
                skip=np.concatenate([L["skip"], np.full(ns, -1, np.int32)]),
                targets=make_targets(T, seed), names={n: nq + j for j, n in enumerate(names)})


@functools.lru_cache(maxsize=None)
def case(kcap, kstride, nq, T, mode, seed=0, with_skip=True, only=None):
    """(lists, (mean, wsum, count, curve)) of one case, computed once and shared by the tests that
    use it; the arrays are read-only."""
    L = make_lists(kcap, kstride, nq, T, seed, only)
    ref = means_ref(L["ids"], L["k"], L["targets"], mode, L["dist"],
                    L["skip"] if with_skip else None, kcap)
    for a in [v for v in L.values() if isinstance(v, np.ndarray)] + list(ref):
        a.setflags(write=False)
    return L, ref


def assert_same(got, want, ctx=""):
    """Equal on the bits where `want` is not NaN, NaN where it is."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, ctx
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), f"{ctx}: a slot that must be NaN is not"
    g, w = got.view(np.int64), want.view(np.int64)
    bad = np.argwhere(~nan & (g != w))
    assert len(bad) == 0, f"{ctx}: {len(bad)} slots differ on their bits, first {bad[:4].tolist()}: " \
                          f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
