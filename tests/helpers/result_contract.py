"""Reference of the result contract (dmlp.h: distance, order, vote, checksum, merge), NumPy and
Python integers only — nothing here calls libdmlp.  tests/test_result_contract_model.py pins it
against the CPU implementations; the GPU contract tests compare kernels with it bit for bit.

  distance  s = 0; for a: d = q[a] - X[:, a]; s = s + d * d    (each step rounded, no FMA)
  order     (dist ascending, id descending); lists padded with (+inf, -1)
  vote      max count, ties -> larger label, no real id -> -1 (ids < 0 are skipped)
  checksum  FNV-1a-64 over the sign-extended label, then id + 1 of every slot of [0, k)
            (a padding id hashes as 0)
"""
from __future__ import annotations

import numpy as np

FNV_OFFSET = 1469598103934665603
FNV_PRIME = 1099511628211
MASK = (1 << 64) - 1
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


# ------------------------------------------------------------------ distance and order
def dist_l2r(q, X):
    """Exact distances of one query to every row: left to right, every step rounded."""
    X = np.asarray(X, np.float64)
    q = np.asarray(q, np.float64)
    s = np.zeros(X.shape[0], np.float64)
    with np.errstate(over="ignore"):
        for a in range(X.shape[1]):
            d = q[a] - X[:, a]
            s = s + d * d
    return s


def dist_r2l(q, X):
    """The same sum taken from the last attribute down (a wrong order, for the model tests)."""
    X = np.asarray(X, np.float64)
    s = np.zeros(X.shape[0], np.float64)
    for a in range(X.shape[1] - 1, -1, -1):
        d = q[a] - X[:, a]
        s = s + d * d
    return s


def dist_pairwise(q, X):
    """The same sum as a balanced tree (another wrong order)."""
    X = np.asarray(X, np.float64)
    d = np.asarray(q, np.float64)[None, :] - X
    t = [d[:, a] * d[:, a] for a in range(X.shape[1])]
    while len(t) > 1:
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0]


def topk_ref(d, k, kstride=None):
    """The first min(k, N) entries of d under (dist asc, id desc), padded to kstride with
    (+inf, -1).  Returns (dist [kstride] f64, ids [kstride] i32)."""
    d = np.asarray(d, np.float64)
    N = d.shape[0]
    kk = max(0, min(int(k), N))
    kstride = max(int(k), 0) if kstride is None else kstride
    ids = np.arange(N, dtype=np.int64)
    order = np.lexsort((-ids, d))[:kk]
    od = np.full(kstride, np.inf, np.float64)
    oi = np.full(kstride, -1, np.int32)
    od[:kk] = d[order]
    oi[:kk] = order
    return od, oi


def knn_ref(X, Qx, k, kstride, dist=dist_l2r):
    """topk_ref of every query: (dist [Q, kstride], ids [Q, kstride])."""
    Q = len(Qx)
    od = np.full((Q, kstride), np.inf, np.float64)
    oi = np.full((Q, kstride), -1, np.int32)
    for q in range(Q):
        od[q], oi[q] = topk_ref(dist(Qx[q], X), k[q], kstride)
    return od, oi


# ------------------------------------------------------------------ vote and checksum
def vote_ref(ids, k, labels) -> int:
    cnt = {}
    for i in range(max(int(k), 0)):
        j = int(ids[i])
        if j >= 0:
            lb = int(labels[j])
            cnt[lb] = cnt.get(lb, 0) + 1
    if not cnt:
        return -1
    best = max(cnt.values())
    return max(lb for lb, c in cnt.items() if c == best)


def fnv_ref(label: int, ids, k) -> int:
    h = FNV_OFFSET
    h = ((h ^ (int(label) & MASK)) * FNV_PRIME) & MASK      # & MASK: the sign extension to u64
    for i in range(max(int(k), 0)):
        h = ((h ^ ((int(ids[i]) + 1) & MASK)) * FNV_PRIME) & MASK
    return h


def finalize_ref(ids, k, labels):
    """(label [Q] i32, checksum [Q] u64) of the lists ids [Q, kstride] with per-query k."""
    Q = len(k)
    lab = np.empty(Q, np.int32)
    cs = np.empty(Q, np.uint64)
    for q in range(Q):
        lab[q] = vote_ref(ids[q], k[q], labels)
        cs[q] = fnv_ref(int(lab[q]), ids[q], k[q])
    return lab, cs


# ------------------------------------------------------------------ merge
def merge_ref(lists_d, lists_i, k, kout):
    """lists_* [L, Q, kin], every list sorted with a padding suffix (id < 0) -> merged
    [Q, kout]: the first min(k_q, kout) real entries of the union under (dist asc, id desc;
    equal keys: the lower list first), then (+inf, -1) up to kout."""
    L, Q, kin = lists_i.shape
    od = np.full((Q, kout), np.inf, np.float64)
    oi = np.full((Q, kout), -1, np.int32)
    for q in range(Q):
        kq = max(0, min(int(k[q]), kout))
        ent = []
        for l in range(L):
            for j in range(min(kq, kin)):
                if lists_i[l, q, j] < 0:
                    break
                ent.append((float(lists_d[l, q, j]), -int(lists_i[l, q, j]), l))
        ent.sort()
        for o, (d, nid, _) in enumerate(ent[:kq]):
            od[q, o], oi[q, o] = d, -nid
    return od, oi


def merge_lists(L, Q, kin, kout, seed=0):
    """L sorted lists per query over disjoint id sets: finite entries, then real entries at +inf,
    then padding.  Query 0: list 0 holds only real +inf entries and every other list only
    padding; query 1: every list is padding."""
    rng = np.random.default_rng(seed)
    lists_d = np.full((L, Q, kin), np.inf, np.float64)
    lists_i = np.full((L, Q, kin), -1, np.int32)
    for q in range(Q):
        perm = rng.permutation(L * kin)
        for l in range(L):
            n_fin = int(rng.integers(0, kin + 1))
            n_inf = int(rng.integers(0, kin - n_fin + 1))
            if q == 0:
                n_fin, n_inf = 0, (kin if l == 0 else 0)
            if q == 1:
                n_fin = n_inf = 0
            ids = perm[l * kin:l * kin + n_fin + n_inf]
            # few distinct distances: ties across lists are ordered by id
            dist = np.concatenate([rng.integers(0, 4, n_fin).astype(np.float64),
                                   np.full(n_inf, np.inf)])
            order = np.lexsort((-ids, dist))
            lists_d[l, q, :len(ids)] = dist[order]
            lists_i[l, q, :len(ids)] = ids[order]
    k = rng.integers(0, kout + 1, Q).astype(np.int32)
    k[:4] = [kout, kout, 0, 1][:min(4, Q)]
    return lists_d, lists_i, k


# ------------------------------------------------------------------ label spaces
def _ends(r, lo=-100):
    def f(N, rng):
        lab = rng.integers(lo, lo + r, N)
        w = rng.integers(0, 4, N)
        lab[w == 0] = lo
        lab[w == 1] = lo + r - 1
        return lab, lo, lo + r
    return f


def _ten(N, rng):
    return rng.integers(0, 10, N), 0, 10


def _two(N, rng):
    return rng.integers(41, 43, N), 41, 43


def _distinct(N, rng):
    return np.arange(N) - 1000, -1000, N - 1000


def _neg(N, rng):
    lab = rng.integers(-300, 0, N)
    lab[:: 7] = -1                       # the real label -1, often
    return lab, -300, 0


def _unknown(N, rng):
    return _neg(N, rng)[0], 0, 0


def _extreme(N, rng):
    return np.array([INT_MIN, -1, 0, INT_MAX])[rng.integers(0, 4, N)], 0, 0


def _extreme_lo(N, rng):
    # the widest range an int pair can state: hi - lo = 2^32 - 1 does not fit an int
    return np.array([INT_MIN, -1, 0, INT_MAX - 1])[rng.integers(0, 4, N)], INT_MIN, INT_MAX


# name -> labels(N, rng) -> (labels, label_lo, label_hi); the range passed contains every label
# or is (0, 0), "not given"
LABEL_SPACES = {
    "ten": _ten, "two": _two, "distinct": _distinct, "r256": _ends(256), "r257": _ends(257),
    "r512": _ends(512), "r513": _ends(513), "neg": _neg, "unknown": _unknown,
    "extreme": _extreme, "extreme_lo": _extreme_lo,
}


def label_space(name: str, N: int, seed: int = 0):
    """(labels [N] int32, label_lo, label_hi) of the named space."""
    lab, lo, hi = LABEL_SPACES[name](N, np.random.default_rng(seed + 17))
    lab = np.ascontiguousarray(lab, np.int64)
    assert (lo, hi) == (0, 0) or (lab.min() >= lo and lab.max() < hi)
    return lab.astype(np.int32), int(lo), int(hi)


# ------------------------------------------------------------------ near-tied neighbours
N_FILL = 2000


def near_tie_input(A: int, P: int, seed: int = 0, extra_queries: int = 4):
    """(X [2000 + P, A], Qx [1 + extra_queries, A], b0): rows [b0, b0 + P) (b0 % 4 == 0) are
    random permutations of one vector base = 500 + s_a 10^u_a, so their distances to the constant
    query 500 are mathematically equal and differ only by the rounding of the left-to-right
    sum; the other rows are uniform in [0, 1000).  Query 0 is the constant one, the rest are
    block rows themselves."""
    assert P % 4 == 0
    rng = np.random.default_rng(seed + 1000 * A + P)
    u = rng.uniform(-3.0, 1.0, A)
    s = rng.choice([-1.0, 1.0], A)
    base = np.round(500.0 + s * 10.0 ** u, 6)
    X = np.round(rng.uniform(0.0, 1000.0, (N_FILL + P, A)), 6)
    b0 = (N_FILL // 2) // 4 * 4
    for r in range(P):
        X[b0 + r] = base[rng.permutation(A)]
    Qx = np.empty((1 + extra_queries, A), np.float64)
    Qx[0] = 500.0
    for j in range(extra_queries):
        Qx[1 + j] = X[b0 + (j * 37) % P]
    return np.ascontiguousarray(X), Qx, b0


# ------------------------------------------------------------------ guarded device buffers
_FILL = {"float64": -7.0, "float32": -7.0, "int32": -12345, "int64": -12345, "uint8": 0xA5}
_BAND = {"float64": -3.0, "float32": -3.0, "int32": -54321, "int64": -54321, "uint8": 0x5A}


class Guarded:
    """A device tensor `t` of `shape` between two sentinel bands (each at least one output row
    and at least 256 bytes, a multiple of 256 bytes so that t keeps the allocation's alignment),
    pre-filled with a second sentinel that no kernel writes."""

    def __init__(self, torch, shape, dtype, fill=None):
        self.torch = torch
        name = str(dtype).replace("torch.", "")
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        item = torch.empty(0, dtype=dtype).element_size()
        n = int(np.prod(shape))
        row = shape[-1] if shape else 1
        per256 = 256 // item
        self.g = (max(row, per256) + per256 - 1) // per256 * per256
        self.fill = _FILL[name] if fill is None else fill
        self.band = _BAND[name]
        assert self.fill != self.band
        self.raw = torch.full((n + 2 * self.g,), self.band, dtype=dtype, device="cuda")
        self.raw[self.g:self.g + n] = self.fill
        self.t = self.raw[self.g:self.g + n].view(shape)
        self.n = n

    def ptr(self):
        return self.t.data_ptr()

    def host(self):
        return self.t.cpu().numpy()

    def check_guards(self, ctx=""):
        self.torch.cuda.synchronize()
        raw = self.raw.cpu().numpy()
        assert (raw[:self.g] == self.band).all(), f"{ctx}: write before the buffer"
        assert (raw[self.g + self.n:] == self.band).all(), f"{ctx}: write past the buffer"

    def untouched(self, mask, ctx=""):
        """asserts that the payload still holds its fill wherever mask (payload-shaped) is set"""
        h = self.host()
        bad = np.argwhere(np.asarray(mask, bool) & (h != self.fill))
        assert len(bad) == 0, f"{ctx}: {len(bad)} slots written that must stay untouched, " \
                              f"first {bad[:4].tolist()}"


def guarded(torch, shape, dtype, fill=None) -> Guarded:
    return Guarded(torch, shape, dtype, fill)
