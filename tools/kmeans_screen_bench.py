#!/usr/bin/env python
"""The screened k-means assignment (csrc/kmeans_screen.hip) against the exact one on one GPU.
tools/kmeans_bench.py's data: uniform rows in [0, 1000)^A, the centroids K rows drawn from them.

  assign   per-iteration cost: kmeans_assign_gpu(X, C, prev) (the fp64 tile over all K) against
           kmeans_assign_gpu(rows, C, prev, screen=True) (centroid prep, screen, pick, escalation)
           on prepared row operands.  Both are compared first: labels, dmin bits, changed.
  rows     kmeans_rows_gpu: the once-per-fit row operands, and the iterations that pay for them.
  stats    candidates per screened row and the escalated share.
  lloyd    one whole iteration either way: assignment against the previous labels, ordered sums,
           the centroid update in place, the changed count read on the host.
Device-event times of windows of back-to-back calls, warmed; within a repeat the candidates
alternate; median, min and max in milliseconds.

    python tools/kmeans_screen_bench.py [--n 100000,1000000] [--a 32,128] [--k 64,256,1024,4096]
                                        [--reps 7] [--inner 3] [--json out.json]
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
    ap.add_argument("--n", default="100000,1000000")
    ap.add_argument("--a", default="32,128")
    ap.add_argument("--k", default="64,256,1024,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=3, help="back-to-back calls per timed window")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)

    import torch
    from distributed_machine_learning_project_amd.ops import knn as K
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_screen_bench needs a GPU")  # no CPU fall-back
    sync = torch.cuda.synchronize

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    def measure(cands):
        for _ in range(a.warmup):
            for fn in cands.values():
                fn()
        t = {n: [] for n in cands}
        for _ in range(a.reps):
            for n, fn in cands.items():
                t[n].append(timed(fn))
        return {n: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                    "max": round(max(v), 4), "n": len(v)} for n, v in t.items()}

    out_rows = []
    rng = np.random.default_rng(0)
    for N in (int(s) for s in a.n.split(",")):
        for A in (int(s) for s in a.a.split(",")):
            X = torch.from_numpy(np.round(rng.uniform(0, 1000, (N, A)), 6)).cuda()
            rows = K.kmeans_rows_gpu(X)
            for Kc in (int(s) for s in a.k.split(",")):
                C = X[torch.from_numpy(np.sort(rng.choice(N, Kc, replace=False))).cuda()]
                C = C.contiguous()
                prev = torch.zeros(N, dtype=torch.int32, device="cuda")
                le, de, ce = K.kmeans_assign_gpu(X, C, prev)
                ls, ds, cs, st = K.kmeans_assign_gpu(rows, C, prev, screen=True, stats=True)
                assert torch.equal(le, ls) and torch.equal(de.view(torch.int64),
                                                           ds.view(torch.int64))
                assert int(ce) == int(cs)
                esc, kept = (int(v) for v in st.cpu())
                row = {"n": N, "a": A, "k": Kc, "escalated_share": esc / N,
                       "mean_candidates": kept / max(N - esc, 1)}
                row["assign"] = measure({
                    "exact_ms": lambda: K.kmeans_assign_gpu(X, C, prev),
                    "screened_ms": lambda: K.kmeans_assign_gpu(rows, C, prev, screen=True)})
                row["rows"] = measure({"prep_rows_ms": lambda: K.kmeans_rows_gpu(X)})
                Cw = C.clone()

                def lloyd(Xa, screen):
                    lab, _, ch = K.kmeans_assign_gpu(Xa, Cw, le, screen=screen)
                    K.cluster_sums_gpu(X, lab, Kc, centroids=Cw)
                    return int(ch)
                row["lloyd"] = measure({"exact_ms": lambda: lloyd(X, False),
                                        "screened_ms": lambda: lloyd(rows, True)})
                out_rows.append(row)
                print(json.dumps(row), flush=True)

    out = {"reps": a.reps, "inner": a.inner, "device": torch.cuda.get_device_name(0),
           "rows": out_rows}
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
