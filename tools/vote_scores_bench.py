#!/usr/bin/env python
"""The class-score kernel against the torch formulation a caller would otherwise write, on one GPU,
over the same device lists: one dmlp_vote_scores launch (counts, scores and the winning label) vs.
gather labels -> scatter_add_ of ones (uniform) or of 1 / d (inverse squared distance) into [Q, C]
-> argmax.  The lists come from one dmlp_knn_local call per k.  Warmed medians of host-clock
windows that end in a device synchronise; the two candidates alternate.  Before anything is timed
the kernel's counts are compared with torch's exactly and its scores to rounding (scatter_add_ sums
in no fixed order; the torch formulation has neither the zero-distance rule nor the tie rule).

    python tools/vote_scores_bench.py [--n 100000] [--q 100000] [--a 32] [--k 16,64]
                                      [--classes 10,300] [--reps 30] [--inner 20] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--q", type=int, default=100000)
    ap.add_argument("--a", type=int, default=32)
    ap.add_argument("--k", default="16,64")
    ap.add_argument("--classes", default="10,300")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)

    import torch
    from distributed_machine_learning_project_amd.ops import knn as K
    if not torch.cuda.is_available():
        raise SystemExit("vote_scores_bench needs a GPU")  # no CPU fall-back: a time from it says nothing
    rng = np.random.default_rng(0)
    X = torch.from_numpy(np.round(rng.uniform(0, 1000, (a.n, a.a)), 6)).cuda()
    Qx = torch.from_numpy(np.round(rng.uniform(0, 1000, (a.q, a.a)), 6)).cuda()
    sync = torch.cuda.synchronize

    def timed(fn):
        # `inner` back-to-back calls per window, so that a short kernel is not timed by the
        # synchronise that ends its window
        sync()
        t = time.perf_counter()
        for _ in range(a.inner):
            fn()
        sync()
        return (time.perf_counter() - t) * 1e3 / a.inner

    def stats(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                "max": round(max(v), 4), "n": len(v)}

    rows = []
    for k in [int(s) for s in a.k.split(",")]:
        kk = np.full(a.q, k, np.int32)
        r = K.knn_gpu(K.prepare_dataset(X), Qx, kk, finalize=False)
        ids, dist = r.ids, r.dist
        idx = ids.long()            # (the torch formulation's index and ones, built once, untimed)
        ones = torch.ones_like(dist)
        kdev = torch.from_numpy(kk).cuda()
        for C in [int(s) for s in a.classes.split(",")]:
            y = torch.from_numpy(rng.integers(0, C, a.n).astype(np.int32)).cuda()
            for weights in ("uniform", "inv_sqdist"):
                def kernel():
                    return K.vote_scores_gpu(ids, kdev, y, 0, C, weights, dist=dist)

                def formulation():
                    lab = y[idx].long()
                    w = ones if weights == "uniform" else 1.0 / dist
                    sc = torch.zeros((a.q, C), dtype=torch.float64, device="cuda")
                    sc.scatter_add_(1, lab, w)
                    return sc, sc.argmax(dim=1)

                cnt, sc, lab = kernel()
                tsc, _ = formulation()
                sync()
                assert int(cnt.sum().item()) == a.q * k, "a kept entry is missing"
                if weights == "uniform":
                    assert torch.equal(sc, tsc), "counts differ from the torch formulation"
                else:
                    assert (dist > 0).all().item(), "a zero distance: the formulations differ"
                    assert torch.allclose(sc, tsc, rtol=1e-12, atol=0), "scores differ"
                assert torch.equal(sc.gather(1, lab.long()[:, None])[:, 0], sc.max(dim=1).values)
                for _ in range(a.warmup):
                    kernel(), formulation()
                t = {"vote_scores_ms": [], "torch_ms": []}
                for _ in range(a.reps):
                    t["vote_scores_ms"].append(timed(kernel))
                    t["torch_ms"].append(timed(formulation))
                row = {"k": k, "classes": C, "weights": weights,
                       "vote_scores_ms": stats(t["vote_scores_ms"]), "torch_ms": stats(t["torch_ms"])}
                row["torch_over_kernel"] = round(
                    row["torch_ms"]["median"] / row["vote_scores_ms"]["median"], 2)
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = {"n": a.n, "q": a.q, "a": a.a, "reps": a.reps, "inner": a.inner,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
