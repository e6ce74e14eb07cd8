#!/usr/bin/env python
"""The k-means kernels (csrc/kmeans.hip) on one GPU.  Uniform rows in [0, 1000)^A, the centroids K
rows drawn from them; for the sums, the labels that assignment gives.

  assign   dmlp_kmeans_assign at both tile widths (dmlp_set_kmeans_tile: 16- and 128-centroid
           tiles) against dmlp_exact_topk at k = 1 on the same rows and centroids.  Before anything
           is timed the two tiles are compared (the same labels and bits) and the top-k's distance
           with dmin (its id differs on ties: its rule is id descending).
  sums     cluster_sums_gpu — the stable sort of the labels, bincount, the offsets, the two
           kernels — and the two kernels alone on a prepared membership, against torch's
           index_add_ + bincount on the same labels (fp64 atomics: other bits from run to run).
  lloyd    one whole iteration: assignment against the previous labels, ordered sums, the
           centroid update in place, the changed count read on the host.
Device-event times of windows of back-to-back calls, warmed; within a repeat the candidates
alternate; median, min and max in milliseconds.

    python tools/kmeans_bench.py [--n 100000,1000000] [--a 32] [--k 8,16,64,256,1024] [--reps 7]
                                 [--inner 3] [--json out.json]
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
    ap.add_argument("--a", type=int, default=32)
    ap.add_argument("--k", default="8,16,64,256,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=3, help="back-to-back calls per timed window")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)

    import torch
    from distributed_machine_learning_project_amd import _lib
    from distributed_machine_learning_project_amd.ops import knn as K
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench needs a GPU")  # no CPU fall-back: its time says nothing
    L = _lib.lib()
    sync = torch.cuda.synchronize
    A = a.a

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

    def with_tile(pj, fn):
        def run():
            old = L.dmlp_set_kmeans_tile(pj)
            try:
                return fn()
            finally:
                L.dmlp_set_kmeans_tile(old)
        return run

    rows = []
    rng = np.random.default_rng(0)
    for N in (int(s) for s in a.n.split(",")):
        X = torch.from_numpy(np.round(rng.uniform(0, 1000, (N, A)), 6)).cuda()
        qidx = torch.arange(N, dtype=torch.int32, device="cuda")
        for Kc in (int(s) for s in a.k.split(",")):
            C = X[torch.from_numpy(np.sort(rng.choice(N, Kc, replace=False))).cuda()].contiguous()
            narrow, wide = (with_tile(pj, lambda: K.kmeans_assign_gpu(X, C)) for pj in (1, 8))
            label, dmin, _ = narrow()
            lw, dw, _ = wide()
            td, _ = K.exact_nearest_gpu(C, X, qidx)
            assert torch.equal(label, lw) and torch.equal(dmin, dw) and torch.equal(dmin, td)
            row = {"n": N, "a": A, "k": Kc, "assign": measure({
                "tile16_ms": narrow, "tile128_ms": wide,
                "exact_topk_k1_ms": lambda: K.exact_nearest_gpu(C, X, qidx)})}

            # the sums: the same membership for the kernels-alone candidate
            perm = torch.sort(label, stable=True).indices.to(torch.int32)
            count = torch.bincount(label.long(), minlength=Kc)
            seg = torch.zeros(Kc + 1, dtype=torch.int64, device="cuda")
            run = torch.zeros(Kc + 1, dtype=torch.int64, device="cuda")
            torch.cumsum(count, 0, out=seg[1:])
            torch.cumsum((count + 63) // 64, 0, out=run[1:])
            nbytes = L.dmlp_cluster_sums_bytes(N, Kc, A + 1)
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            sums = torch.zeros((Kc, A + 1), dtype=torch.float64, device="cuda")
            lab64 = label.long()

            def kernels():
                _lib.check(L.dmlp_cluster_sums(X.data_ptr(), N, A, Kc, dmin.data_ptr(),
                                               perm.data_ptr(), seg.data_ptr(), run.data_ptr(),
                                               ws.data_ptr(), nbytes, sums.data_ptr(), None,
                                               K._stream()), "cluster sums")

            def index_add():
                s = torch.zeros((Kc, A + 1), dtype=torch.float64, device="cuda")
                s[:, :A].index_add_(0, lab64, X)
                s[:, A].index_add_(0, lab64, dmin)
                return s, torch.bincount(lab64, minlength=Kc)
            kernels()
            full = K.cluster_sums_gpu(X, label, Kc, dmin)[0]
            assert torch.equal(full, sums)
            row["max_rel_diff_index_add"] = float(
                ((index_add()[0] - sums).abs() / sums.abs().clamp_min(1e-300)).max().item())
            row["sums"] = measure({
                "cluster_sums_ms": lambda: K.cluster_sums_gpu(X, label, Kc, dmin),
                "kernels_only_ms": kernels, "index_add_ms": index_add})

            Cw = C.clone()

            def lloyd():
                lab, dm, ch = K.kmeans_assign_gpu(X, Cw, label)
                K.cluster_sums_gpu(X, lab, Kc, centroids=Cw)
                return int(ch)
            row["lloyd"] = measure({"iteration_ms": lloyd})
            rows.append(row)
            print(json.dumps(row), flush=True)

    out = {"a": A, "reps": a.reps, "inner": a.inner, "device": torch.cuda.get_device_name(0),
           "rows": rows}
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
