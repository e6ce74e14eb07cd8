"""Reference and inputs of the radius search (dmlp.h: dmlp_radius_count / dmlp_radius_fill /
dmlp_radius_sort), NumPy only — nothing here calls libdmlp.  tests/test_radius_model.py pins it
against the CPU twins, ops.reference.radius_reference and the k-NN reference (a query's neighbours
are the first count entries of its k-NN list at k = count); tests/test_radius.py compares the
kernels with it bit for bit.

  membership  point n is a neighbour of q iff dist_l2r(q, x_n) <= r2[q]   (r2 a SQUARED radius; the
              boundary included; a negative or NaN r2 keeps nothing, +inf every point)
  fill        the neighbours in DESCENDING id order
  sort        (dist asc, id desc)
"""
from __future__ import annotations

import functools

import numpy as np

import result_contract as RC

NS = (1, 127, 128, 129, 300)        # both sides of the 128-point tile
QS = (1, 63, 64, 65, 130)           # both sides of a workgroup's 64 queries
AS = (1, 2, 7, 32, 33, 130)         # an odd tail, the double2 path, a second LDS chunk
NEAR_TIE_AS = (7, 32, 33, 130)
N_R2 = 14                           # length of the per-query rotation of radii


def reference(X, Qx, r2, dist=RC.dist_l2r):
    """(count int32 [Q], sorted, desc): per query the (dist, ids) of its neighbours ordered by (dist
    asc, id desc), and by descending id."""
    count = np.zeros(len(Qx), np.int32)
    srt, desc = [], []
    for q in range(len(Qx)):
        d = dist(Qx[q], X)
        with np.errstate(invalid="ignore"):
            ids = np.flatnonzero(d <= r2[q])
        order = ids[np.lexsort((-ids, d[ids]))]
        count[q] = len(ids)
        srt.append((d[order], order.astype(np.int32)))
        desc.append((d[ids[::-1]], ids[::-1].astype(np.int32)))
    return count, srt, desc


def csr_offsets(count):
    """(off int64 [Q], total) of the exclusive prefix sum."""
    indptr = np.zeros(len(count) + 1, np.int64)
    np.cumsum(count, out=indptr[1:])
    return np.ascontiguousarray(indptr[:-1]), int(indptr[-1])


def expected(segs, off, size, fill_d, fill_i, count=None):
    """Flat (dist float64 [size], ids int32 [size]) holding the segments at their offsets and the
    fills everywhere else; count (default: the segments' lengths) cuts a segment to its first
    count[q] entries."""
    d = np.full(size, fill_d, np.float64)
    i = np.full(size, fill_i, np.int32)
    for q, (sd, si) in enumerate(segs):
        c = len(si) if count is None else int(count[q])
        d[off[q]:off[q] + c] = sd[:c]
        i[off[q]:off[q] + c] = si[:c]
    return d, i


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _radii(X, Qx, rot):
    """Per-query r2 rotating through: negative, 0, NaN, +inf, below every distance, and the exact
    distance of the query's 1st, 17th and last neighbour with nextafter of each in both
    directions."""
    r2 = np.empty(len(Qx), np.float64)
    inf = np.inf
    for q in range(len(Qx)):
        ds = np.sort(RC.dist_l2r(Qx[q], X))
        d1, d17, dl = ds[0], ds[min(16, len(ds) - 1)], ds[-1]
        r2[q] = (-1.0, 0.0, np.nan, inf, np.nextafter(d1, -inf),
                 d1, np.nextafter(d1, inf), d17, np.nextafter(d17, -inf), np.nextafter(d17, inf),
                 dl, np.nextafter(dl, -inf), np.nextafter(dl, inf),
                 np.nextafter(d17, -inf) if d17 > 0 else 0.5)[(q + rot) % N_R2]
    return r2


@functools.lru_cache(maxsize=None)
def grid_case(N, Q, A, rot=0, huge=True):
    """(X [N, A], Qx [Q, A], r2 [Q]): coarse-grid rows with values in {0, 1, 2} — distances are
    small integers with many ties —, a block of up to 30 identical rows, every fifth query a dataset
    row (zero distances) and, with `huge`, one row with a coordinate of 1e200: real points at
    distance +inf, kept only by r2 = +inf."""
    rng = np.random.default_rng(1000 * N + 10 * Q + A)
    X = rng.integers(0, 3, (N, A)).astype(np.float64)
    b = min(30, N // 2)
    X[N // 4:N // 4 + b] = X[N // 4]
    if huge and N >= 3:
        X[N - 2, A - 1] = 1e200
    Qx = rng.integers(0, 3, (Q, A)).astype(np.float64)
    Qx[::5] = X[rng.integers(0, max(1, N - 2), len(Qx[::5]))]
    r2 = _radii(X, Qx, rot)
    for a in (X, Qx, r2):
        a.setflags(write=False)
    return X, Qx, r2


@functools.lru_cache(maxsize=None)
def all_equal_case(N=300, Q=65, A=7):
    """Every row and query the same vector and r2 = 0: every point is a hit of every query, so each
    offer round of a point column holds 16 hits per query."""
    X = np.full((N, A), 1.25)
    Qx = np.full((Q, A), 1.25)
    r2 = np.zeros(Q)
    r2[1::3] = -0.0
    r2[2::7] = np.nextafter(0.0, -1.0)      # below every distance: nothing
    for a in (X, Qx, r2):
        a.setflags(write=False)
    return X, Qx, r2


@functools.lru_cache(maxsize=None)
def near_tie_case(A):
    """result_contract.near_tie_input(A, 160): the block's distances to query 0 are mathematically
    equal and differ by the rounding of the left-to-right sum alone; r2[0] is the middle distinct
    value of them, so the membership depends on the summation order.  The other queries (block
    rows) take their 17th neighbour's distance."""
    X, Qx, b0 = RC.near_tie_input(A, 160)
    d0 = RC.dist_l2r(Qx[0], X)[b0:b0 + 160]
    u = np.unique(d0)
    r2 = np.array([np.sort(RC.dist_l2r(Qx[q], X))[16] for q in range(len(Qx))])
    r2[0] = u[len(u) // 2]
    for a in (X, Qx, r2):
        a.setflags(write=False)
    return X, Qx, r2, b0


@functools.lru_cache(maxsize=None)
def ref_of(kind, *args):
    """reference() of a named case, computed once and shared."""
    case = {"grid": grid_case, "equal": all_equal_case, "tie": near_tie_case}[kind](*args)
    return reference(*case[:3])


# (N, Q, A) of the kernel tests: every N with every Q (A rotating), and every A on the largest
SHAPES = [(N, Q, AS[(i + 2 * j) % len(AS)]) for i, N in enumerate(NS) for j, Q in enumerate(QS)] + \
         [(300, 130, A) for A in AS]
SHAPES = list(dict.fromkeys(SHAPES))
