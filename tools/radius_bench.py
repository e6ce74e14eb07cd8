#!/usr/bin/env python
"""The radius search's three launches — dmlp_radius_count, dmlp_radius_fill, dmlp_radius_sort
(csrc/radius.hip) — timed separately on one GPU against dmlp_exact_topk at k = 16 on the same
device rows: the count pass runs that kernel's distance tile without its candidate buffers and
compactions.  Uniform data; per target count (16, 256) one squared radius for every query, bisected
until a sample of the queries has that mean count.  Device-event
times of windows of back-to-back calls, warmed; within a repeat the calls alternate (count, top-k,
fill, sort — the sort always gets freshly filled segments); median, min and max over the repeats.
Before anything is timed the counts are checked against the k-NN lists of the sample.

Then, as a time only, the chunked torch formulation a caller would otherwise write on the same
rows: ((Qc[:, None] - X[None]) ** 2).sum(-1) <= r2 followed by nonzero, on the first --torch-q
queries in chunks of --torch-chunk.

    python tools/radius_bench.py [--n 100000] [--a 32] [--q 1024,16384,131072] [--counts 16,256]
                                 [--reps 7] [--inner 2] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--a", type=int, default=32)
    ap.add_argument("--q", default="1024,16384,131072")
    ap.add_argument("--counts", default="16,256")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=2, help="back-to-back calls per timed window")
    ap.add_argument("--sample", type=int, default=1024, help="queries that set the radii")
    ap.add_argument("--torch-q", type=int, default=1024)
    ap.add_argument("--torch-chunk", type=int, default=32)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)

    import torch
    from distributed_machine_learning_project_amd import _lib
    from distributed_machine_learning_project_amd.ops import knn as K
    if not torch.cuda.is_available():
        raise SystemExit("radius_bench needs a GPU")  # no CPU fall-back: a time from it says nothing
    L = _lib.lib()
    rng = np.random.default_rng(0)
    qs = [int(s) for s in a.q.split(",")]
    X = torch.from_numpy(np.round(rng.uniform(0, 1000, (a.n, a.a)), 6)).cuda()
    Qall = torch.from_numpy(np.round(rng.uniform(0, 1000, (max(qs), a.a)), 6)).cuda()
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

    # the radii: bisected on the sample's mean count, from its distances to the c-th neighbours
    ns = min(a.sample, max(qs))
    targets = [int(s) for s in a.counts.split(",")]
    cmax = max(targets)
    r = K.knn_gpu(ds, Qall[:ns], np.full(ns, cmax, np.int32), finalize=False, exact=True)
    radii = {}
    for c in targets:
        lo, hi = float(r.dist[:, c - 1].min().item()), float(r.dist[:, c - 1].max().item())
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            if K.radius_count_gpu(ds, Qall[:ns], mid).sum().item() < c * ns:
                lo = mid
            else:
                hi = mid
        radii[c] = hi
    for c, r2 in radii.items():   # the counts of the sample agree with its k-NN lists
        got = K.radius_count_gpu(ds, Qall[:ns], r2)
        want = (r.dist <= r2).sum(dim=1).to(torch.int32)
        full = want == cmax       # (the list ends before the radius does: only a lower bound)
        assert bool(((got == want) | (full & (got >= want))).all().item()), "counts differ"

    rows = []
    for Q in qs:
        Qx = Qall[:Q].contiguous()
        qidx = torch.arange(Q, dtype=torch.int32, device="cuda")
        k16 = torch.full((Q,), 16, dtype=torch.int32, device="cuda")
        td = torch.empty((Q, 16), dtype=torch.float64, device="cuda")
        ti = torch.empty((Q, 16), dtype=torch.int32, device="cuda")

        def topk():
            _lib.check(L.dmlp_exact_topk(X.data_ptr(), a.n, a.a, Qx.data_ptr(), qidx.data_ptr(),
                                         k16.data_ptr(), Q, 16, td.data_ptr(), ti.data_ptr(), 16,
                                         stream()), "exact topk")
        for c, r2 in radii.items():
            r2d = torch.full((Q,), r2, dtype=torch.float64, device="cuda")
            cnt = torch.zeros(Q, dtype=torch.int32, device="cuda")

            def count():
                _lib.check(L.dmlp_radius_count(X.data_ptr(), a.n, a.a, Qx.data_ptr(), Q,
                                               r2d.data_ptr(), cnt.data_ptr(), stream()), "count")
            count()
            indptr = torch.zeros(Q + 1, dtype=torch.int64, device="cuda")
            torch.cumsum(cnt, 0, out=indptr[1:])
            total = int(indptr[Q].item())
            od = torch.empty(max(total, 1), dtype=torch.float64, device="cuda")
            oi = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
            nbytes = L.dmlp_radius_sort_bytes(total, Q)
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

            def fill():
                _lib.check(L.dmlp_radius_fill(X.data_ptr(), a.n, a.a, Qx.data_ptr(), Q,
                                              r2d.data_ptr(), cnt.data_ptr(), indptr.data_ptr(),
                                              od.data_ptr(), oi.data_ptr(), stream()), "fill")

            def sort():
                _lib.check(L.dmlp_radius_sort(od.data_ptr(), oi.data_ptr(), cnt.data_ptr(),
                                              indptr.data_ptr(), Q, ws.data_ptr(), nbytes,
                                              stream()), "sort")
            for _ in range(a.warmup):
                count(), topk(), fill(), sort()
            t = {"count_ms": [], "topk16_ms": [], "fill_ms": [], "sort_ms": []}
            for _ in range(a.reps):
                t["count_ms"].append(timed(count))
                t["topk16_ms"].append(timed(topk))
                t["fill_ms"].append(timed(fill))
                t["sort_ms"].append(timed(sort, 1))
            row = {"Q": Q, "target_count": c, "r2": r2, "mean_count": round(total / Q, 2),
                   "max_count": int(cnt.max().item()), **{n: stats(v) for n, v in t.items()}}
            row["count_over_topk16"] = round(row["count_ms"]["median"] /
                                             row["topk16_ms"]["median"], 3)
            row["fill_over_count"] = round(row["fill_ms"]["median"] /
                                           row["count_ms"]["median"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del od, oi, ws

    # the torch formulation, a time only
    tq = min(a.torch_q, max(qs))
    form = []
    for c, r2 in radii.items():
        def formulation():
            out = []
            for s in range(0, tq, a.torch_chunk):
                Qc = Qall[s:s + a.torch_chunk]
                out.append((((Qc[:, None] - X[None]) ** 2).sum(-1) <= r2).nonzero())
            return out
        formulation()
        v = [timed(formulation, 1) for _ in range(max(3, a.reps // 2))]
        form.append({"Q": tq, "chunk": a.torch_chunk, "target_count": c, "torch_ms": stats(v)})
        print(json.dumps(form[-1]), flush=True)

    out = {"n": a.n, "a": a.a, "reps": a.reps, "inner": a.inner,
           "device": torch.cuda.get_device_name(0), "rows": rows, "torch_formulation": form}
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
