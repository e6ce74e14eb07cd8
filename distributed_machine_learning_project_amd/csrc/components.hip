// components.hip — connected components of the radius graph: rows i and j of X are linked iff
// d(x_i, x_j) <= r2 (r2 ONE squared radius, the boundary inclusive), d the reference's fp64 distance
// (fp64_tile.h), which is symmetric bit for bit: (a - b) and (b - a) differ in sign only.  comp[i]
// is the smallest row id of i's component — a pure function of the inputs, although atomics build
// it.  Three launches, no workspace: comp is the union-find's parent array.
//   k_comp_init     comp[i] = i, *status = 0
//   k_comp_link     the distance tile of radius.hip with the rows as their own queries, lower
//                   triangle only: workgroup b serves rows 64 b .. and scans points [0, 64 b + 64),
//                   offering a pair when p < q.  A lane with a hit unites q and p in comp[].
//   k_comp_flatten  comp[i] = root(i)
// The union-find is lock-free: find both roots, hook the LARGER root under the SMALLER with a
// compare-exchange (larger: larger -> smaller), on failure go on from the value it returned.  So
// parent[x] <= x always, with equality only at roots: no cycles, every walk ends, and a tree's root
// is its smallest id.  Every access to comp[] in the link kernel is a relaxed agent-scope atomic
// (workgroups on other XCDs do not see plain stores within a kernel); no fence is needed, since the
// algorithm relies on the atomicity of single words alone: a stale read costs a failed exchange
// and another round.  No path compression: a parent only ever changes at a root.
#include "dmlp.h"
#include "fp64_tile.h"
#include <limits.h>

namespace {

using Rd = dmlp::Fp64Tile<64, 8, 16>;
static_assert(Rd::RI * Rd::PJ <= 32, "a lane's hits of one tile are kept in a 32-bit mask");

__device__ __forceinline__ int parent_of(const int* comp, int x) {
  return __hip_atomic_load(comp + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Unites the sets of a and b; returns the root both hang under from now on, or -1 after `cap`
// steps.  Every step lowers a or b (a parent is smaller than its child, and a failed exchange
// returns the new, smaller parent of a), so a + b < 2 N bounds the steps: the cap cannot be
// reached while parent[x] <= x holds.  It turns a bug into an error code instead of a hang.
__device__ __forceinline__ int unite(int* comp, int a, int b, unsigned cap, int* status) {
  for (unsigned it = 0; it < cap; ++it) {
    if (a == b) return a;
    if (a < b) { const int t = a; a = b; b = t; }
    const int pa = parent_of(comp, a);
    if (pa != a) { a = pa; continue; }
    const int pb = parent_of(comp, b);
    if (pb != b) { b = pb; continue; }
    int seen = a;  // both were roots when read: hook the larger under the smaller
    if (__hip_atomic_compare_exchange_strong(comp + a, &seen, b, __ATOMIC_RELAXED,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return b;
    a = seen;  // somebody hooked a first: go on from its new parent
  }
  __hip_atomic_store(status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return -1;
}

__global__ __launch_bounds__(256) void k_comp_init(int* __restrict__ comp, int N,
                                                   int* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) comp[i] = i;
  if (i == 0) *status = 0;
}

// HEAVY_FIRST: workgroup b scans 64 b + 64 points, so the last ones are the longest; they are
// started first (HIP promises no dispatch order; observed, blocks start in index order).
template <bool HEAVY_FIRST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_comp_link(
    const double* __restrict__ X, int N, int A, double r2, int* comp, int* status) {
  constexpr int QB = Rd::QB, PJ = Rd::PJ, PT = Rd::PT, AS = Rd::AS, RI = Rd::RI;
  __shared__ __attribute__((aligned(16))) double Qs[QB][AS];
  __shared__ __attribute__((aligned(16))) double Xs[PT][AS];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int b = HEAVY_FIRST ? (int)(gridDim.x - 1 - blockIdx.x) : (int)blockIdx.x;
  const int q0 = b * QB;
  const int end = N - q0 < QB ? N : q0 + QB;   // the points below this workgroup's last row
  const unsigned cap = 2u * (unsigned)N + 64u;
  // the last root seen for row ty + 16 i: an ancestor of the row stays one for good (parents change
  // at roots only), so the next unite of the row starts there instead of at the row
  int cur[RI];
#pragma unroll
  for (int i = 0; i < RI; ++i) cur[i] = q0 + ty + 16 * i;

  dmlp::fp64_tile_scan<Rd>(
      X, (int64_t)end, A, X, q0, N, Qs, Xs, [](int qi) { return qi; },
      [&](int64_t p0, const double (&acc)[RI][PJ]) __attribute__((always_inline)) {
        // this lane's hits of the tile as a mask, bit i PJ + j: pad rows (q >= N) hold zeros and
        // are no rows; p < q < N keeps the pad points of the last tile out as well.  A NaN or
        // negative r2 is >= no distance.
        unsigned hits = 0;
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
          for (int j = 0; j < PJ; ++j) {
            const int q = q0 + ty + 16 * i;
            const int64_t p = p0 + tx + 16 * j;
            hits |= (p < q && q < N && acc[i][j] <= r2 ? 1u : 0u) << (i * PJ + j);
          }
        // divergent from here to the end of the offer: no barrier and no wave-wide operation
        while (hits) {
          const int bit = __ffs(hits) - 1;
          hits &= hits - 1;
          const int i = bit / PJ, p = (int)p0 + tx + 16 * (bit % PJ);
          int c = cur[0];
#pragma unroll
          for (int u = 1; u < RI; ++u) c = i == u ? cur[u] : c;
          const int r = unite(comp, c, p, cap, status);
#pragma unroll
          for (int u = 0; u < RI; ++u) cur[u] = (i == u && r >= 0) ? r : cur[u];
        }
      });
}

// A launch of its own, so every hook of the link kernel is visible.  In place: whatever a walk
// meets in comp[] while other threads write their roots — a parent or already a root — is an
// ancestor of where it stands, so it ends at the same root.
__global__ __launch_bounds__(256) void k_comp_flatten(int* comp, int N, int* status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int x = i;
  for (int it = 0; it <= N; ++it) {   // a walk is shorter than N steps
    const int p = parent_of(comp, x);
    if (p == x) {
      __hip_atomic_store(comp + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    x = p;
  }
  __hip_atomic_store(status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int g_heavy_first = 1;

}  // namespace

extern "C" int dmlp_set_components_order(int heavy_first) {
  const int old = g_heavy_first;
  g_heavy_first = heavy_first ? 1 : 0;
  return old;
}

extern "C" int dmlp_radius_components(const double* X, int64_t N, int A, double r2, int* comp,
                                      int* status, void* stream) {
  if (N <= 0) return 0;
  if (N > INT_MAX || A < 1 || !X || !comp || !status) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)N;
  const dim3 flat((unsigned)((N + 255) / 256)), tiles((unsigned)((N + Rd::QB - 1) / Rd::QB));
  hipLaunchKernelGGL(k_comp_init, flat, dim3(256), 0, st, comp, n, status);
  DMLP_LAUNCH_CHECK();
  if (g_heavy_first)
    hipLaunchKernelGGL(k_comp_link<true>, tiles, dim3(256), 0, st, X, n, A, r2, comp, status);
  else
    hipLaunchKernelGGL(k_comp_link<false>, tiles, dim3(256), 0, st, X, n, A, r2, comp, status);
  DMLP_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_comp_flatten, flat, dim3(256), 0, st, comp, n, status);
  DMLP_LAUNCH_CHECK();
  return 0;
}
