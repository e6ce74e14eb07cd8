"""The pair screen's fill check once per ring iteration (csrc/screen_x1.hip k_screen_x1 PERIOD).

Under the pair epilogue the screen appends once per two steps and tests its sub-buffers' fill once
per four (two appends), against a reserve of two slots: a sub-buffer found with 14 entries goes to
16 = SUB before the next test.  The data here fill the sub-buffers as fast as the kernel allows:

  ordered   points on one axis in (x, -x) pairs, their radius falling with the row index, queries
            next to the origin: every 8-row group beats every group before it, so every pair of
            steps is a hit in every column and every sub-buffer takes both appends of an iteration;
  one_kg    the same, with the falling radii on the rows of one row group (kg = 0) only and every
            other row far out: all hits of a column fall on one sub-buffer;
  ties      64 pairs of points at the origin, one pair per group of 64 groups: more groups tie
            for the best key than a column may keep, and the overflow must be reported
            (cand_cnt = -1).

Every value is a small integer and the centre is 0 exactly, so the fp16 operands, the products and
the fp32 sums are exact in any order and a NumPy model reproduces the kernel's keys bit for bit.
The model (model_lists) follows the kernel's own sequence — the appends per pair, the check behind
every second pair, the wave-wide compaction with the 15-bit radix select, the re-deal of the kept
entries, the append behind the last check — and records the fullest sub-buffer it saw: the CPU
cases show that these data do take one from 14 to 16, and that the kept set is the one the final
threshold alone gives (the k-th largest key of everything, low bit cleared, minus 2 eps).  The GPU
cases compare what dmlp_screen_x1 and dmlp_screen_x1_early wrote with it — counts, thresholds and
the sets of (key, group) entries — and the native step's neighbours with the CPU oracle's.

Q = 64 and 65 (a second workgroup of one column), A = 32, k = 16, N = 2048 and 4096."""
import functools
import os
import sys

import numpy as np
import pytest

from distributed_machine_learning_project_amd import _lib
from distributed_machine_learning_project_amd.ops import knn as K

HERE = os.path.dirname(os.path.abspath(__file__))
for _d in (HERE, os.path.join(HERE, "helpers")):
    if _d not in sys.path:
        sys.path.insert(0, _d)
import test_screen_contract as TSC  # noqa: E402  (Ops and the runners of the C ABI)
import x1_contract as X1  # noqa: E402

A, KQ, SUB, RESERVE = 32, 16, 16, 2
CAPE = 4 * (SUB - RESERVE)
KINDS = ("ordered", "one_kg", "ties")
SHAPES = [(kind, N, Q) for kind in KINDS for N in (2048, 4096) for Q in (64, 65)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.lib()
    return torch


@functools.lru_cache(maxsize=None)
def case(kind: str, N: int, Q: int):
    """(X, labels, Qx, k, reference), built once per shape and never modified."""
    g = np.random.default_rng(N + Q)
    x0 = np.zeros(N)
    sign = np.where(np.arange(N) & 1, -1.0, 1.0)
    if kind == "ordered":
        x0 = sign * (N // 2 - np.arange(N) // 2)           # radii N/2 .. 1, each as (r, -r)
    else:
        # the rows that must not hit: further out at every step (never above a threshold once
        # there is one), 2 apart so that only a few of their groups share a 16-bit key
        x0 = sign * (1100.0 + 2.0 * (np.arange(N) // 16))
        if kind == "one_kg":
            rows = np.nonzero(((np.arange(N) & 15) >> 2) == 0)[0]   # rows 0 - 3 of every step
            # radii up to 1024, 4 (N = 2048) or 2 apart: the best groups' keys lie further apart
            # than the 2 eps band, a column keeps exactly k entries at a compaction and its one
            # busy sub-buffer restarts from an even count
            step = 2048.0 / len(rows)
            x0[rows] = sign[rows] * step * (len(rows) // 2 - np.arange(len(rows)) // 2)
        else:
            # the first row of 64 different 8-row groups of row group 0, spread over the scan;
            # its (x, -x) partner moves to the origin with it
            gi = np.arange(64) * (N // 8 // 64)
            r0 = X1.group_rows(gi, 8)[:, 0]
            x0[r0] = x0[r0 + 1] = 0.0
    X = np.zeros((N, A))
    X[:, 0] = x0
    Qx = np.zeros((Q, A))
    Qx[:, 0] = g.integers(-3, 4, Q)
    Qx[:, 1] = g.integers(0, 4, Q)
    k = np.full(Q, KQ, np.int32)
    labels = g.integers(0, 10, N).astype(np.int32)
    ref = X1.reference(X, Qx, k, hl=1)
    assert (ref.mu == 0.0).all(), "the centre must be 0 exactly"
    return X, labels, Qx, k, ref


def model_lists(ref):
    """(sets, cnt, h, peak): per query the set of (key, group) entries the pair screen (one
    slice, SUB = 16) leaves, its count (-1: overflow), its final threshold as fp32, and the
    largest number of entries any sub-buffer held at a check."""
    Q, P = ref.Q, ref.n_tiles * 2                           # pairs of steps
    gm = X1.group_max(ref.a_model.astype(np.float32), ref.n_tiles, 8)   # exact: integers / 2
    assert (gm[np.isfinite(gm)] == X1.group_max(ref.a_model, ref.n_tiles, 8)[np.isfinite(gm)]).all()
    keys = X1.key16(gm)
    sets, cnts, hs, peak = [None] * Q, np.zeros(Q, np.int32), np.zeros(Q, np.float32), 0
    lowest = np.float32(-np.finfo(np.float32).max)
    two = np.float32(2.0)
    for w0 in range(0, Q, 64):                              # one wave per 64 columns
        cols = range(w0, min(Q, w0 + 64))
        h = {c: lowest for c in cols}
        flag = {c: False for c in cols}
        buf = {c: [] for c in cols}                         # buffered group indices
        cnt = {c: [0, 0, 0, 0] for c in cols}

        def compact(final):
            for c in cols:
                ks = keys[c, buf[c]]
                if not flag[c] and len(ks) >= KQ:
                    kth = int(np.sort(ks)[-KQ]) & ~1        # the 15-bit radix select's floor
                    ak = np.float32(X1.decode16(kth))
                    h[c] = max(h[c], np.float32(ak - two * ref.eps[c]))
                kh = X1.key16(np.array([h[c]], np.float32))[0]
                kept = [g_ for g_, k_ in zip(buf[c], ks) if k_ >= kh]
                if flag[c] or len(kept) > CAPE:
                    flag[c], kept = True, []
                    h[c] = np.float32(np.inf)
                buf[c] = kept
                n = len(kept)
                cnt[c] = [(n + 3) >> 2, (n + 2) >> 2, (n + 1) >> 2, n >> 2]
                if final:
                    cnts[c] = -1 if flag[c] else n
                    sets[c] = {(int(keys[c, g_]), int(g_)) for g_ in kept}

        for p in range(P):
            for c in cols:
                for kg in range(4):
                    g_ = 4 * p + kg
                    if gm[c, g_] >= h[c]:                   # (padding: -inf; overflowed: h = +inf)
                        buf[c].append(g_)
                        cnt[c][kg] += 1
            if p % 2 == 0:                                  # the check behind every second pair
                top = max(max(cnt[c]) for c in cols)
                peak = max(peak, top)
                assert top <= SUB, "a sub-buffer past its last slot"
                if top > SUB - RESERVE:
                    compact(False)
        final_h = dict(h)
        compact(True)
        for c in cols:
            hs[c] = h[c] if cnts[c] >= 0 else final_h[c]
    return sets, cnts, hs, peak


@functools.lru_cache(maxsize=None)
def model(kind, N, Q):
    return model_lists(case(kind, N, Q)[4])


# ------------------------------------------------------------------ CPU: the data and the model
@pytest.mark.parametrize("kind,N,Q", SHAPES)
def test_model_fills_sub_buffers(kind, N, Q):
    """The data take a sub-buffer from 14 entries to SUB = 16 between two checks, and the model's
    kept set is the one the final threshold alone gives, whatever the cadence was."""
    ref = case(kind, N, Q)[4]
    sets, cnt, h, peak = model(kind, N, Q)
    if kind == "ties":
        assert (cnt == -1).all()
        return
    assert peak == SUB, f"fullest sub-buffer at a check: {peak}"
    assert (cnt >= KQ).all() and (cnt <= CAPE).all()
    gm = X1.group_max(ref.a_model.astype(np.float32), ref.n_tiles, 8)
    keys = X1.key16(gm)
    for q in range(Q):
        real = np.nonzero(gm[q] > -np.inf)[0]
        kth = int(np.sort(keys[q, real])[-KQ]) & ~1
        hq = np.float32(np.float32(X1.decode16(kth)) - np.float32(2.0) * ref.eps[q])
        assert hq == h[q]
        kh = X1.key16(np.array([hq], np.float32))[0]
        assert sets[q] == {(int(keys[q, g_]), int(g_)) for g_ in real if keys[q, g_] >= kh}


# ------------------------------------------------------------------ GPU: the screen's lists
def check_against_model(ls, kind, N, Q, ctx):
    sets, cnt_m, h_m, _ = model(kind, N, Q)
    ids, cnt, h = ls.host()
    np.testing.assert_array_equal(cnt[:, 0], cnt_m, err_msg=f"{ctx}: counts")
    for q in range(Q):
        if cnt_m[q] < 0:
            continue
        assert h[q, 0, 0] == h_m[q], f"{ctx}: threshold of query {q}"
        e = ids[q, 0, :cnt[q, 0]]
        got = set(zip(X1.entry_key(e).tolist(), X1.entry_group(e).tolist()))
        assert len(got) == cnt[q, 0], f"{ctx}: duplicate entries of query {q}"
        assert got == sets[q], f"{ctx}: candidate set of query {q}"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,Q", SHAPES)
def test_lists_equal_model(torch_cuda, kind, N, Q):
    """dmlp_screen_x1 (one slice) and dmlp_screen_x1_early (every ready word preset) write the
    model's counts, thresholds and candidate sets; ties report the overflow."""
    X, labels, Qx, k, ref = case(kind, N, Q)
    ops = TSC.Ops(torch_cuda, ref, labels)
    assert TSC.grows_of(ops.L, ref, KQ) == 8 and ops.L.dmlp_screen_x1_cap_kt(ref.KT, KQ) == CAPE + 4
    check_against_model(TSC.run_x1(ops, KQ, 1), kind, N, Q, f"{kind} N={N} Q={Q} plain")
    ls, estats = TSC.run_x1_early(ops, KQ, rdy_tiles=max(1, ref.n_tiles // 8))
    assert estats[0] == 0 and estats[2] == 0
    check_against_model(ls, kind, N, Q, f"{kind} N={N} Q={Q} early")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,Q", SHAPES)
def test_step_equals_oracle(torch_cuda, kind, N, Q):
    """The native step on the same data: neighbours, distances, votes and checksums equal the CPU
    oracle's bit for bit (the step picks its own slices: a tied query that overflows one escalates natively)."""
    X, labels, Qx, k, ref = case(kind, N, Q)
    r = K.step(X, labels, (0, 10), Qx, k, k_range=(KQ, KQ), lists=True)
    torch_cuda.cuda.synchronize()
    assert r.early_timeouts == 0
    np.testing.assert_array_equal(r.ids.cpu().numpy(), ref.nn_i)
    np.testing.assert_array_equal(r.dist.cpu().numpy().view(np.uint64), ref.nn_d.view(np.uint64))
    lab_ref, cs_ref = K.finalize_cpu(ref.nn_i, k, labels)
    np.testing.assert_array_equal(r.label.cpu().numpy(), lab_ref)
    np.testing.assert_array_equal(r.checksum.cpu().numpy().view(np.uint64), cs_ref)
