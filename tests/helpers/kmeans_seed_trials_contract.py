"""Plain NumPy reference of dmlp.h's "k-means seeding, local trials" and the tests' shared cases."""
import functools

import numpy as np

import kmeans_seed_contract as SC
from kmeans_seed_contract import INF, LAST, R, bits, sum_lr, walk  # noqa: F401


def ref_seed_trials(X, K, L, i0, u):
    """(seeds, C, w, the steps at which the least potential was met by more than one trial)"""
    N = len(X)

    def trial(p, w):
        with np.errstate(invalid="ignore"):
            d = R.distances(X, X[p])
        m = np.where(d < w, d, w)
        v = np.where(m < INF, m, 0.0)
        runs = [sum_lr(v[r:r + 64]) for r in range(0, N, 64)]
        blocks = [sum_lr(runs[b:b + 64]) for b in range(0, len(runs), 64)]
        return m, v, runs, blocks, sum_lr(blocks)

    def pick(v, runs, blocks, T, uj):
        if not 0 < T < INF:
            return int(uj * N)
        t = uj * T
        b, s = walk(blocks, 0.0, t)
        r, s = walk(runs[64 * b:64 * b + 64], s, t)
        r += 64 * b
        return 64 * r + walk(v[64 * r:64 * r + 64], s, t)[0]

    seeds, ties = np.full(K, i0, np.int32), 0
    cur = trial(i0, np.full(N, INF))
    for j in range(1, K):
        cands = [pick(*cur[1:], u[j - 1][l]) for l in range(L)]
        trials = [trial(p, cur[0]) for p in cands]
        P = [t[4] for t in trials]
        best = P.index(min(P))                          # the smallest l with the least P_l
        ties += P.count(P[best]) > 1
        seeds[j], cur = cands[best], trials[best]
    return seeds, X[seeds].copy(), cur[0], ties


# (N, A, K, L, data): data as seed_case's, "-dup": column 2 of u repeats column 0 (one row twice
# per step).  L = 1: the D^2 seeding; run, block and stage edges with L at its cap and off the
# compiled bounds; ties between potentials; a NaN row and a +inf row
OLD = [(65, 33, 9, 1, "int"), (4097, 130, 2, 1, "int"), (8257, 33, 9, 1, "gauss")]
TIES = [(65, 33, 9, 4, "int"), (130, 2, 9, 4, "equal"), (130, 33, 9, 4, "gauss-dup")]
CASES = OLD + [(63, 1, 9, 2, "gauss"), (65, 130, 9, 5, "gauss"), (4097, 1, 9, 3, "gauss"),
               (8257, 33, 9, 16, "gauss"), (8257, 130, 2, 7, "int")] + TIES + [
                   (130, 33, 9, 3, "nonfinite")]


@functools.lru_cache(maxsize=None)
def trials_case(N, A, K, L, data):
    """(X, i0, u [K - 1, L], the reference's result); u: seed_case's at L = 1, else 0.0, LAST first"""
    X, i0, u1, _ = SC.seed_case(N, A, K, data.split("-")[0])
    u = np.random.default_rng(26 + L).random((K - 1, L))    # (L = 4: every case of TIES ties)
    if L == 1:
        u = u1.reshape(K - 1, 1).copy()
    else:
        u[0, :2] = [0.0, LAST]
    if data.endswith("-dup"):
        u[:, 2] = u[:, 0]
    return X, i0, u, ref_seed_trials(X, K, L, i0, u)


def check(got, ref):
    """(seeds, C, w) as host arrays against another such triple: the same rows, the same bits"""
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(bits(got[1]), bits(ref[1]))
    np.testing.assert_array_equal(bits(got[2]), bits(ref[2]))
