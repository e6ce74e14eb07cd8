// kmeans.hip — the two halves of a Lloyd iteration (dmlp.h: k-means), both pure functions of their
// inputs and bit-identical to the host twins: no FMA, no floating-point atomics.
//
//   k_kmeans_assign<PJ>   label[i] = the smallest c minimising d(x_i, C_c), d the reference's fp64
//     distance (fp64_tile.h).  The tile runs with the ROWS as its queries (64 per workgroup) and
//     the K centroids as its data stream (kmeans_tile.h: the body, shared with the screened
//     assignment's escalation kernel), PJ = 8 (128-centroid tiles, radius.hip's shape) or PJ = 1
//     (16-centroid tiles: K = 8 or 16 pays for 16 columns, not 128).  None of the top-k tier's
//     selection: a lane keeps ONE running (d, c) per row, taken by a strict < while its columns
//     arrive in ascending c, so it holds its smallest c of the least distance; a NaN distance is
//     < nothing and so ranks as +inf.  A row's 16 lanes sit in one wave: one lexicographic (d, c)
//     minimum over them by four xor-shuffles ends the row, as k_radius's count reduction does.
//     Lane tx == 0 writes label and dmin and compares with prev; a wave counts its changed rows by
//     ballot + popcount and adds them to *changed once (an integer atomic).  No LDS beyond the
//     tile's staging.  A row without a finite distance takes label 0; its dmin (+inf or NaN, as
//     computed) is formed again by dmlp::exact_dist, the same operations in the same order.
//   k_cluster_run_sums    cluster c's members in ascending row id (perm: the stable sort of the
//     labels) are cut into runs of 64; one wave sums one run.  The wave loads the run's 64 perm
//     entries in one load, lane L owns column L (+ 64 per further pass when T > 64), and the walk
//     takes the members in order: a member's id comes out of the perm register by a lane
//     broadcast, so its row address is wave-uniform and its row one coalesced read, and the loads
//     of kAhead members are issued before the first of their dependent adds.  One run per wave
//     whatever A: the pass is bound by the row reads, which idle lanes do not slow, and the
//     estimator's T = A + 1 = 33 at A = 32 does not fit half a wave anyway.
//   k_cluster_finish      one wave per cluster, lanes as columns: the cluster's run partials summed
//     in run order into sums[c, :], and on request the Lloyd step: centroid c = sums[c, :A] /
//     (double)count, IEEE division; an empty cluster keeps its centroid.
#include "dmlp.h"
#include "kmeans_tile.h"
#include <limits.h>
#include <math.h>

namespace {

template <int PJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PJ == 1 ? 4 : 2))) void
k_kmeans_assign(const double* __restrict__ X, int N, int A, const double* __restrict__ Cn, int K,
                const int* __restrict__ prev, int* __restrict__ label, double* __restrict__ dmin,
                int* changed) {
  dmlp::kmeans_assign_tile<PJ>(X, A, Cn, K, prev, label, dmin, changed, blockIdx.x * 64, N,
                               [](int qi) { return qi; });
}

__global__ void k_kmeans_zero(int* p) { *p = 0; }

constexpr int kSumWaves = 4;   // waves per workgroup of the two sum kernels
constexpr int kRunAhead = 8;   // member rows in flight ahead of the add chain
constexpr int kFinAhead = 32;  // run partials in flight: K waves only, so latency is all there is

// sum_{j < n} val(j), left to right from 0.0, the loads of AHEAD terms issued before their adds
// (n wave-uniform; val(j) must be loadable for every j < n)
template <int AHEAD, class Val>
__device__ __forceinline__ double ordered_sum(int64_t n, Val val) {
  double s = 0.0;
  for (int64_t j0 = 0; j0 < n; j0 += AHEAD) {
    double v[AHEAD];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) v[u] = val(j0 + u < n ? j0 + u : j0);
#pragma unroll
    for (int u = 0; u < AHEAD; ++u)
      if (j0 + u < n) s = __dadd_rn(s, v[u]);
  }
  return s;
}

// partial[r, :] = the ordered sum of run r's value rows, r < min(run_off[K], rcap)
__global__ __launch_bounds__(64 * kSumWaves) void k_cluster_run_sums(
    const double* __restrict__ X, int N, int A, const double* __restrict__ extra,
    const int* __restrict__ perm, const int64_t* __restrict__ seg_off,
    const int64_t* __restrict__ run_off, int K, int T, int64_t rcap,
    double* __restrict__ partial) {
  const int lane = dmlp::lane_id();
  const int64_t r = (int64_t)blockIdx.x * kSumWaves + (threadIdx.x >> 6);
  const int64_t R = run_off[K] < rcap ? run_off[K] : rcap;
  if (r >= R) return;   // (wave-uniform)
  // the run's cluster: the last c with run_off[c] <= r (empty clusters repeat an offset)
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (run_off[mid] <= r) lo = mid; else hi = mid;
  }
  const int64_t m0 = seg_off[lo] + 64 * (r - run_off[lo]);
  int64_t n = seg_off[lo + 1] - m0;
  n = n > 64 ? 64 : n;
  if (m0 < 0 || m0 + n > N) n = 0;   // offsets that do not describe perm: an all-zero partial
  const int pm = lane < n ? perm[m0 + lane] : 0;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int col = t0 + lane;
    const double s = ordered_sum<kRunAhead>(n, [&](int64_t j) __attribute__((always_inline)) {
      const int id = __builtin_amdgcn_readlane(pm, (int)j);   // wave-uniform: a scalar row base
      if ((unsigned)id >= (unsigned)N) return 0.0;            // no row: never read
      return col < A ? X[(int64_t)id * A + col] : (col < T ? extra[id] : 0.0);
    });
    if (col < T) partial[r * T + col] = s;
  }
}

// sums[c, :] = the ordered sum of cluster c's run partials; cio (nullable): the Lloyd step
__global__ __launch_bounds__(64 * kSumWaves) void k_cluster_finish(
    const double* __restrict__ partial, const int64_t* __restrict__ seg_off,
    const int64_t* __restrict__ run_off, int K, int A, int T, int64_t rcap,
    double* __restrict__ sums, double* __restrict__ cio) {
  const int lane = dmlp::lane_id();
  const int c = blockIdx.x * kSumWaves + (threadIdx.x >> 6);
  if (c >= K) return;   // (wave-uniform)
  const int64_t r0 = run_off[c];
  const int64_t r1 = run_off[c + 1] < rcap ? run_off[c + 1] : rcap;
  const int64_t cnt = seg_off[c + 1] - seg_off[c];
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int col = t0 + lane;
    const double s = ordered_sum<kFinAhead>(
        r0 < 0 ? 0 : r1 - r0, [&](int64_t j) __attribute__((always_inline)) {
          return col < T ? partial[(r0 + j) * T + col] : 0.0;
        });
    if (col < T) sums[(int64_t)c * T + col] = s;
    if (cio != nullptr && cnt > 0 && col < A) cio[(int64_t)c * A + col] = __ddiv_rn(s, (double)cnt);
  }
}

using dmlp::kAssignNarrowK;   // (kmeans_tile.h)
int g_assign_pj = 0;   // 0: by K; 1 / 8: that tile (tools/kmeans_bench.py)

int64_t max_runs(int64_t N, int K) { return N / 64 + K; }   // sum_c ceil(n_c / 64) <= N / 64 + K

}  // namespace

extern "C" int dmlp_set_kmeans_tile(int pj) {
  const int old = g_assign_pj;
  g_assign_pj = pj == 1 || pj == 8 ? pj : 0;
  return old;
}

extern "C" int dmlp_kmeans_assign(const double* X, int64_t N, int A, const double* C, int K,
                                  const int* prev, int* label, double* dmin, int* changed,
                                  void* stream) {
  if (N <= 0 || K <= 0) return 0;
  // (K: a tile's pad columns past the last centroid stay inside an int)
  if (N > INT_MAX || K > INT_MAX - 128 || A < 1 || !X || !C || !label || !dmin ||
      (changed && !prev))
    return -1;
  hipStream_t st = (hipStream_t)stream;
  if (changed) {
    hipLaunchKernelGGL(k_kmeans_zero, dim3(1), dim3(1), 0, st, changed);
    DMLP_LAUNCH_CHECK();
  }
  const dim3 grid((unsigned)((N + 63) / 64));
  const int pj = g_assign_pj ? g_assign_pj : (K <= kAssignNarrowK ? 1 : 8);
  if (pj == 1)
    hipLaunchKernelGGL(k_kmeans_assign<1>, grid, dim3(256), 0, st, X, (int)N, A, C, K, prev, label,
                       dmin, changed);
  else
    hipLaunchKernelGGL(k_kmeans_assign<8>, grid, dim3(256), 0, st, X, (int)N, A, C, K, prev, label,
                       dmin, changed);
  DMLP_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t dmlp_cluster_sums_bytes(int64_t N, int K, int T) {
  if (N < 0 || N > INT_MAX || K < 0 || T < 1) return -1;
  return max_runs(N, K) * T * (int64_t)sizeof(double);
}

extern "C" int dmlp_cluster_sums(const double* X, int64_t N, int A, int K, const double* extra,
                                 const int* perm, const int64_t* seg_off, const int64_t* run_off,
                                 void* ws, int64_t ws_bytes, double* sums, double* centroids_io,
                                 void* stream) {
  if (N <= 0 || K <= 0) return 0;
  if (N > INT_MAX || A < 1 || !X || !perm || !seg_off || !run_off || !ws || !sums) return -1;
  const int T = A + (extra ? 1 : 0);
  const int64_t rcap = max_runs(N, K);
  if (ws_bytes < dmlp_cluster_sums_bytes(N, K, T)) return -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_cluster_run_sums, dim3((unsigned)((rcap + kSumWaves - 1) / kSumWaves)),
                     dim3(64 * kSumWaves), 0, st, X, (int)N, A, extra, perm, seg_off, run_off, K, T,
                     rcap, (double*)ws);
  DMLP_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cluster_finish, dim3((unsigned)((K + kSumWaves - 1) / kSumWaves)),
                     dim3(64 * kSumWaves), 0, st, (const double*)ws, seg_off, run_off, K, A, T, rcap,
                     sums, centroids_io);
  DMLP_LAUNCH_CHECK();
  return 0;
}
