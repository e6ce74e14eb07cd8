#!/usr/bin/env python
"""The weighted vote curve against what it replaces, on one GPU: one dmlp_vote_curve_weighted launch
(inverse squared distance) over a set of sorted neighbour lists vs. the loop of kcap label-only
dmlp_vote_scores launches (one per k) over the same lists, and vs. one uniform dmlp_vote_curve
launch.  Warmed medians of host-clock windows that end in a device synchronise; the candidates
alternate.  The weighted curve's columns are compared with the dmlp_vote_scores outputs, and its
mode 0 with the uniform curve, before anything is timed.

    python tools/weighted_vote_curve_bench.py [--n 100000] [--q 100000] [--a 32] [--kcap 64]
                                              [--labels 10] [--reps 30] [--inner 20] [--json out.json]
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
    ap.add_argument("--kcap", type=int, default=64)
    ap.add_argument("--labels", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20, help="curve launches per timed window")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)

    import torch
    from distributed_machine_learning_project_amd import _lib
    from distributed_machine_learning_project_amd.ops import knn as K
    if not torch.cuda.is_available():
        raise SystemExit("weighted_vote_curve_bench needs a GPU")  # a CPU time says nothing
    L = _lib.lib()
    rng = np.random.default_rng(0)
    X = torch.from_numpy(np.round(rng.uniform(0, 1000, (a.n, a.a)), 6)).cuda()
    Qx = torch.from_numpy(np.round(rng.uniform(0, 1000, (a.q, a.a)), 6)).cuda()
    y = torch.from_numpy(rng.integers(0, a.labels, a.n).astype(np.int32)).cuda()
    truth = torch.from_numpy(rng.integers(0, a.labels, a.q).astype(np.int32)).cuda()
    ds = K.prepare_dataset(X, y, (0, a.labels))
    kk = np.full(a.q, a.kcap, np.int32)
    sync = torch.cuda.synchronize
    r = K.knn_gpu(ds, Qx, kk, finalize=False)
    ids, dist = r.ids, r.dist
    kdev = [torch.full((a.q,), k, dtype=torch.int32, device="cuda") for k in range(1, a.kcap + 1)]
    lab = torch.empty(a.q, dtype=torch.int32, device="cuda")
    cols = torch.empty((a.kcap, a.q), dtype=torch.int32, device="cuda")
    st = K._stream()

    def scores_loop(keep=False):
        for j in range(a.kcap):
            out = cols[j] if keep else lab
            rc = L.dmlp_vote_scores(dist.data_ptr(), ids.data_ptr(), a.kcap, kdev[j].data_ptr(), a.q,
                                    None, y.data_ptr(), 0, a.labels, 1, None, None, out.data_ptr(),
                                    st)
            assert rc == 0

    def weighted():
        return K.vote_curve_gpu(ids, kdev[-1], y, a.kcap, dist=dist, weights="inv_sqdist",
                                lists=False)

    def weighted_hits():
        return K.vote_curve_gpu(ids, kdev[-1], y, a.kcap, dist=dist, weights="inv_sqdist",
                                lists=False, truth=truth)

    def uniform():
        return K.vote_curve_gpu(ids, kdev[-1], y, a.kcap)

    scores_loop(keep=True)
    got, hits, _ = weighted_hits()
    uni = uniform()[0]
    uni_w = K.vote_curve_gpu(ids, kdev[-1], y, a.kcap, score=True)[0]    # mode 0 of the new kernel
    sync()
    assert torch.equal(got, cols.t()), "the weighted curve's columns differ from dmlp_vote_scores"
    assert torch.equal(hits, (cols == truth[None, :]).sum(dim=1)), "hits differ"
    assert torch.equal(uni, uni_w), "mode 0 differs from the uniform curve"
    differ = int((got != uni).sum())

    def timed(fn, inner=1):
        # `inner` back-to-back calls per window, so that a short kernel is not timed by the
        # synchronise that ends its window
        sync()
        t = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        return (time.perf_counter() - t) * 1e3 / inner

    for _ in range(a.warmup):
        scores_loop(), weighted(), weighted_hits(), uniform()
    t = {"scores_loop_ms": [], "weighted_curve_ms": [], "weighted_curve_hits_ms": [],
         "uniform_curve_ms": []}
    for _ in range(a.reps):
        t["scores_loop_ms"].append(timed(scores_loop))
        t["weighted_curve_ms"].append(timed(weighted, a.inner))
        t["uniform_curve_ms"].append(timed(uniform, a.inner))
        t["weighted_curve_hits_ms"].append(timed(weighted_hits, a.inner))
    out = {"n": a.n, "q": a.q, "a": a.a, "kcap": a.kcap, "labels": a.labels, "reps": a.reps,
           "inner": a.inner, "device": torch.cuda.get_device_name(0),
           "slots_weighted_differs_from_uniform": differ}
    for key, v in t.items():
        out[key] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                    "max": round(max(v), 4), "n": len(v)}
    out["speedup_weighted_vs_scores_loop"] = round(
        out["scores_loop_ms"]["median"] / out["weighted_curve_ms"]["median"], 2)
    out["ratio_weighted_vs_uniform"] = round(
        out["weighted_curve_ms"]["median"] / out["uniform_curve_ms"]["median"], 2)
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
