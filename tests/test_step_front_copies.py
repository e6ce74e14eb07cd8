"""The native step's front (csrc/pipeline.hip dmlp_step) in its reduced form — the query norms
carried by the last fragment chunk's copy, a uniform k handed to the screen as a scalar with its
array copied behind the operands' event, the step's words cleared by the previous call's tail —
against the exact CPU path, bit for bit: the sorted (distance, id) lists, the votes, the checksums
and the report text.

Shapes: N = 4096, A = 32; Q below the number of query chunks (1, 3, 5), with chunk boundaries
that are no multiple of 4 queries (257), and 4096; k uniform with the bounds given and scanned,
mixed 1-16 (the array stays in front of the screen) and k = 1.  Sequences on one workspace: a
smaller Q over a larger buffer behind a tail that cleared the words, a call rejected before it
touched anything, a step that fell back to the device image, and a process's first call."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, A, QMAX, KS = 4096, 32, 4096, 16
QS = (1, 3, 5, 257, 4096)
# name -> (k of the queries, k_range handed to the step or None to have it scanned)
KCFG = {
    "uniform_given": (lambda k: np.full_like(k, 16), (16, 16)),
    "uniform_scanned": (lambda k: np.full_like(k, 16), None),
    "mixed_1_16": (lambda k: k, (1, 16)),
    "k_one": (lambda k: np.ones_like(k), (1, 1)),
}


@functools.lru_cache(maxsize=None)
def data():
    import distributed_machine_learning_project_amd as dmlp
    return dmlp.generate(N, QMAX, A, 0.0, 1000.0, 1, 16, 10, seed=1507)


@functools.lru_cache(maxsize=None)
def reference(kname):
    """(k, dist, ids, label, checksum) of all QMAX queries, computed once per k configuration; a
    case with fewer queries takes the first Q rows (each query's result is its own)."""
    from distributed_machine_learning_project_amd.ops import knn as K
    inp = data()
    k = np.ascontiguousarray(KCFG[kname][0](inp.k), np.int32)
    d, i = K.knn_cpu(inp.X, inp.Qx, k, kstride=KS)
    lab, cs = K.finalize_cpu(i, k, inp.labels)
    for a in (k, d, i, lab, cs):
        a.setflags(write=False)
    return k, d, i, lab, cs


def check(st, dst, Qx, k, d_ref, i_ref, lab_ref, cs_ref, what, path=0, escalate_ok=False):
    import distributed_machine_learning_project_amd as dmlp
    Q = len(k)
    assert st.path == path, what
    assert st.early_timeouts == 0, what
    assert escalate_ok or st.n_escalated == 0, what
    live = np.arange(KS)[None, :] < k[:, None]
    d, i = st.dist.cpu().numpy(), st.ids.cpu().numpy()
    assert np.array_equal(i[live], i_ref[live]), f"{what}: neighbour ids"
    assert np.array_equal(d[live].view(np.uint64), d_ref[live].view(np.uint64)), f"{what}: distances"
    assert np.array_equal(st.label.cpu().numpy(), lab_ref), f"{what}: votes"
    assert np.array_equal(st.checksum.cpu().numpy().view(np.uint64), cs_ref), f"{what}: checksums"
    assert bytes(dst[:st.report_len]) == dmlp.format_report(cs_ref), f"{what}: report text"
    assert Qx.shape[0] == Q


def run_step(kname, Q, report_bytes=None):
    """One step over the first Q queries under k configuration kname, checked."""
    import torch
    from distributed_machine_learning_project_amd.ops import knn as K
    inp = data()
    k, d, i, lab, cs = reference(kname)
    dst = torch.empty(report_bytes or 48 * Q + 64, dtype=torch.uint8).pin_memory().numpy()
    st = K.step(inp.X, inp.labels, (0, 10), inp.Qx[:Q], k[:Q], k_range=KCFG[kname][1],
                report=dst, lists=True, kstride=KS)
    check(st, dst, inp.Qx[:Q], k[:Q], d[:Q], i[:Q], lab[:Q], cs[:Q], f"{kname} Q={Q}")
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("kname", list(KCFG))
def test_step_matches_cpu(kname, Q):
    run_step(kname, Q)


@pytest.mark.gpu
def test_smaller_q_behind_a_cleared_tail():
    """Two steps at Q = 4096, then Q = 257 in the same (larger) operand buffers: the second and
    third calls run on words the previous call's tail cleared, and the third finds its norms at
    another offset of the joined allocation."""
    run_step("uniform_given", 4096)
    run_step("mixed_1_16", 4096)
    run_step("uniform_given", 257)
    run_step("mixed_1_16", 257)


@pytest.mark.gpu
def test_rejected_call_then_good_call():
    """A report buffer below the bound is rejected (-2) before the step touches its workspace;
    the next call is served as usual."""
    run_step("uniform_given", 257)
    with pytest.raises(RuntimeError, match=r"code -2\b"):
        run_step("uniform_given", 257, report_bytes=64)
    run_step("uniform_given", 257)
    run_step("mixed_1_16", 5)


@pytest.mark.gpu
def test_device_image_fallback_then_good_step():
    """Queries outside the fp16 screen's range: the step falls back to the device image path
    (path 2) after its front was issued, and neither it nor the following step on the host
    operands may see words the other left behind."""
    import torch
    from distributed_machine_learning_project_amd.ops import knn as K
    inp = data()
    run_step("uniform_given", 257)
    Qf = np.ascontiguousarray(inp.Qx[:64] * 1000.0)  # up to 1e6: |q - centre| >= 65504
    kf = np.full(64, 16, np.int32)
    d, i = K.knn_cpu(inp.X, Qf, kf, kstride=KS)
    lab, cs = K.finalize_cpu(i, kf, inp.labels)
    dst = torch.empty(48 * 64 + 64, dtype=torch.uint8).pin_memory().numpy()
    st = K.step(inp.X, inp.labels, (0, 10), Qf, kf, k_range=(16, 16), report=dst, lists=True,
                kstride=KS)
    # (far-off queries may overflow the device image's screen and escalate: still exact)
    check(st, dst, Qf, kf, d, i, lab, cs, "queries outside the fp16 range", path=2,
          escalate_ok=True)
    run_step("uniform_given", 257)
    run_step("mixed_1_16", 257)


@pytest.mark.gpu
def test_first_call_of_a_fresh_workspace():
    """The workspace lives as long as the process: a child process's first step (nothing vouches
    for its words), then a second one behind it."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fresh workspace ok" in r.stdout


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    run_step("uniform_given", 257)
    run_step("uniform_scanned", 4096)
    print("fresh workspace ok")
