#!/usr/bin/env python
"""The radius-graph components kernel (dmlp_radius_components, csrc/components.hip) and DBSCAN.fit
on one GPU.  Uniform data; per target mean count (16, 256) one squared radius, bisected until a
sample of the rows has that mean count (the row itself counted).

  kernel   dmlp_radius_components — heaviest workgroups first (the default) and in row order —
           against dmlp_radius_count with the rows as their own queries (twice the distance work,
           no unions), and against itself at r2 = -1 (the same distance work, no union at all: the
           difference is what the unions cost).  Device-event times of windows of back-to-back
           calls, warmed; within a repeat the candidates alternate; median, min and max.
  fit      DBSCAN(r2, min_samples).fit from host rows, wall clock with a device sync, against the
           way to the same labels without the components kernel: radius_gpu's unsorted CSR copied
           to the host, components of the core rows there (scipy's connected_components where it
           imports, else min-label propagation in NumPy), border rows from the CSR's distances.
           The labels of the two are compared before anything is timed.

    python tools/components_bench.py [--n 100000] [--a 32] [--counts 16,256] [--reps 7]
                                     [--inner 2] [--fit-reps 3] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_components(indptr, ids, N):
    """comp[i] = smallest id of i's component, from a symmetric CSR; (comp, how)."""
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import connected_components
        g = csr_matrix((np.ones(len(ids), np.int8), ids, indptr), shape=(N, N))
        _, lab = connected_components(g, directed=False)
        first = np.full(lab.max() + 1 if N else 0, N, np.int64)
        np.minimum.at(first, lab, np.arange(N))
        return first[lab].astype(np.int32), "scipy"
    except ImportError:
        comp = np.arange(N, dtype=np.int64)
        seg = indptr[:-1][np.diff(indptr) > 0]
        rows = np.flatnonzero(np.diff(indptr) > 0)
        while True:
            new = comp.copy()
            new[rows] = np.minimum(comp[rows], np.minimum.reduceat(comp[ids], seg))
            new = new[new]
            if (new == comp).all():
                return comp.astype(np.int32), "numpy"
            comp = new


def baseline_fit(K, torch, X, r2, ms):
    """The labels of DBSCAN.fit from the radius search's CSR and host components."""
    Xd = torch.from_numpy(X).cuda()
    ds = K.prepare_dataset(Xd)
    count = K.radius_count_gpu(ds, Xd, r2)
    return labels_of_csr(*(t.cpu().numpy() for t in
                           K.radius_gpu(ds, Xd, r2, sort=False, count=count)), ms)


def labels_of_csr(indptr, d, ids, ms):
    """(labels, how): DBSCAN's labels from the CSR of the rows' neighbours within r2."""
    N = len(indptr) - 1
    rows = np.repeat(np.arange(N), np.diff(indptr))
    is_core = np.diff(indptr) >= ms
    core = np.flatnonzero(is_core)
    rank = np.cumsum(is_core) - 1
    cc = is_core[rows] & is_core[ids]                     # core-core edges, in core ranks
    cptr = np.zeros(len(core) + 1, np.int64)
    np.cumsum(np.bincount(rank[rows[cc]], minlength=len(core)), out=cptr[1:])
    comp, how = host_components(cptr, rank[ids[cc]], len(core))
    core_labels = np.unique(comp, return_inverse=True)[1].ravel()
    labels = np.full(N, -1, np.int32)
    labels[core] = core_labels
    nb = ~is_core[rows] & is_core[ids]                    # a non-core row's core neighbours
    r, i, dd = rows[nb], ids[nb], d[nb]
    order = np.lexsort((-i, dd, r))                       # per row: (dist asc, id desc)
    r, i = r[order], i[order]
    head = np.ones(len(r), bool)
    head[1:] = r[1:] != r[:-1]
    labels[r[head]] = core_labels[rank[i[head]]]
    return labels, how


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--a", type=int, default=32)
    ap.add_argument("--counts", default="16,256")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=2, help="back-to-back calls per timed window")
    ap.add_argument("--sample", type=int, default=1024, help="rows that set the radii")
    ap.add_argument("--fit-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)

    import torch
    from distributed_machine_learning_project_amd import _lib
    from distributed_machine_learning_project_amd.models import DBSCAN
    from distributed_machine_learning_project_amd.ops import knn as K
    if not torch.cuda.is_available():
        raise SystemExit("components_bench needs a GPU")  # no CPU fall-back: its time says nothing
    L = _lib.lib()
    rng = np.random.default_rng(0)
    Xh = np.round(rng.uniform(0, 1000, (a.n, a.a)), 6)
    X = torch.from_numpy(Xh).cuda()
    N, A = a.n, a.a
    sync = torch.cuda.synchronize
    ds = K.prepare_dataset(X)
    stream = K._stream

    def timed(fn, inner=None):
        inner = inner or a.inner
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / inner

    def stats(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                "max": round(max(v), 4), "n": len(v)}

    # the radii: bisected on the mean count of a sample of the rows (the row itself counts)
    ns = min(a.sample, N)
    targets = [int(s) for s in a.counts.split(",")]
    r = K.knn_gpu(ds, X[:ns], np.full(ns, max(targets), np.int32), finalize=False, exact=True)
    radii = {}
    for c in targets:
        lo, hi = float(r.dist[:, c - 1].min().item()), float(r.dist[:, c - 1].max().item())
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            if K.radius_count_gpu(ds, X[:ns], mid).sum().item() < c * ns:
                lo = mid
            else:
                hi = mid
        radii[c] = hi

    comp = torch.empty(N, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
    rows = []
    for c, r2 in radii.items():
        r2d = torch.full((N,), r2, dtype=torch.float64, device="cuda")

        def components(rr=r2):
            _lib.check(L.dmlp_radius_components(X.data_ptr(), N, A, rr, comp.data_ptr(),
                                                status.data_ptr(), stream()), "components")

        def row_order():
            old = L.dmlp_set_components_order(0)
            try:
                components()
            finally:
                L.dmlp_set_components_order(old)

        def no_unions():
            components(-1.0)

        def count():
            _lib.check(L.dmlp_radius_count(X.data_ptr(), N, A, X.data_ptr(), N, r2d.data_ptr(),
                                           cnt.data_ptr(), stream()), "count")
        # the two block orders agree, and the status word is clear
        components()
        first = comp.clone()
        row_order()
        assert bool((first == comp).all().item()) and int(status.item()) == 0
        cands = {"components_ms": components, "components_row_order_ms": row_order,
                 "components_no_unions_ms": no_unions, "count_ms": count}
        for _ in range(a.warmup):
            for fn in cands.values():
                fn()
        t = {n: [] for n in cands}
        for _ in range(a.reps):
            for n, fn in cands.items():
                t[n].append(timed(fn))
        count()
        row = {"target_count": c, "r2": r2, "mean_count": round(float(cnt.sum().item()) / N, 2),
               "n_components": int(torch.unique(first).numel()),
               **{n: stats(v) for n, v in t.items()}}
        med = {n: row[n]["median"] for n in cands}
        row["components_over_count"] = round(med["components_ms"] / med["count_ms"], 3)
        row["row_order_over_heavy_first"] = round(med["components_row_order_ms"] /
                                                  med["components_ms"], 3)
        row["unions_ms"] = round(med["components_ms"] - med["components_no_unions_ms"], 4)
        rows.append(row)
        print(json.dumps(row), flush=True)

    # DBSCAN.fit end to end, wall clock
    fits = []
    for c, r2 in radii.items():
        ms = max(2, c // 2)
        want, how = baseline_fit(K, torch, Xh, r2, ms)
        db = DBSCAN(r2=r2, min_samples=ms, device="gpu").fit(Xh)
        assert np.array_equal(db.labels_, want), "DBSCAN.fit and the CSR baseline differ"

        def wall(fn):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            return (time.perf_counter() - t0) * 1e3
        t = {"fit_ms": [], "csr_baseline_ms": []}
        for _ in range(a.fit_reps):
            t["fit_ms"].append(wall(lambda: DBSCAN(r2=r2, min_samples=ms, device="gpu").fit(Xh)))
            t["csr_baseline_ms"].append(wall(lambda: baseline_fit(K, torch, Xh, r2, ms)))
        row = {"target_count": c, "r2": r2, "min_samples": ms, "n_clusters": db.n_clusters_,
               "n_core": int(len(db.core_sample_indices_)), "n_noise": int((want == -1).sum()),
               "host_components": how, **{n: stats(v) for n, v in t.items()}}
        row["baseline_over_fit"] = round(row["csr_baseline_ms"]["median"] /
                                         row["fit_ms"]["median"], 2)
        fits.append(row)
        print(json.dumps(row), flush=True)

    out = {"n": N, "a": A, "reps": a.reps, "inner": a.inner,
           "device": torch.cuda.get_device_name(0), "kernel": rows, "fit": fits}
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
