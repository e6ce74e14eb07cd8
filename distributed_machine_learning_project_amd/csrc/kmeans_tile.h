// kmeans_tile.h — the exact fp64 assignment of one 64-row workgroup, shared by k_kmeans_assign
// (kmeans.hip: the rows in order) and k_kmeans_escalate (kmeans_screen.hip: the rows of a list).
#pragma once
#include "fp64_tile.h"
#include <limits.h>
#include <math.h>

namespace dmlp {

// Centroid counts up to this take the 16-centroid tile: the largest measured K at which it beats
// the 128-centroid tile (profiles/kmeans.md: ahead at K = 8, 16 and 64, behind at 256 and 1024;
// nothing in between was measured)
constexpr int kAssignNarrowK = 64;

// Slots q0 .. q0 + 64 of nq, slot qi standing for row qrow(qi) of X: label, dmin and the compare
// with prev of those rows.  The tile runs with the ROWS as its queries and the K centroids as its
// data stream, PJ = 8 (128-centroid tiles) or PJ = 1 (16-centroid tiles).  A lane keeps ONE
// running (d, c) per row, taken by a strict < while its columns arrive in ascending c, so it holds
// its smallest c of the least distance; a NaN distance is < nothing and so ranks as +inf.  A row's
// 16 lanes sit in one wave: one lexicographic (d, c) minimum over them by four xor-shuffles ends
// the row.  Lane tx == 0 writes label and dmin and compares with prev; a wave counts its changed
// rows by ballot + popcount and adds them to *changed once (an integer atomic).  A row without a
// finite distance takes label 0; its dmin (+inf or NaN, as computed) is formed again by
// dmlp::exact_dist, the same operations in the same order.  All 256 threads call it together.
template <int PJ, class QRow>
__device__ __forceinline__ void kmeans_assign_tile(const double* __restrict__ X, int A,
                                                   const double* __restrict__ Cn, int K,
                                                   const int* __restrict__ prev,
                                                   int* __restrict__ label,
                                                   double* __restrict__ dmin, int* changed, int q0,
                                                   int nq, QRow qrow) {
  using Tl = Fp64Tile<64, PJ, 16>;
  constexpr int QB = Tl::QB, PT = Tl::PT, AS = Tl::AS, RI = Tl::RI;
  __shared__ __attribute__((aligned(16))) double Qs[QB][AS];
  __shared__ __attribute__((aligned(16))) double Xs[PT][AS];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  // this lane's best of slot ty + 16 i so far: never a NaN, +inf until a finite distance arrives
  double bd[RI];
  int bc[RI];
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    bd[i] = INFINITY;
    bc[i] = INT_MAX;
  }

  fp64_tile_scan<Tl>(
      Cn, (int64_t)K, A, X, q0, nq, Qs, Xs, qrow,
      [&](int64_t p0, const double (&acc)[RI][PJ]) __attribute__((always_inline)) {
        // columns c = p0 + tx + 16 j ascend over j and over the tiles: strict < keeps the smaller
        // c of equal distances; pads (c >= K) are no centroids; NaN < x is false
#pragma unroll
        for (int j = 0; j < PJ; ++j) {
          const int c = (int)p0 + tx + 16 * j;
#pragma unroll
          for (int i = 0; i < RI; ++i) {
            const bool take = c < K && acc[i][j] < bd[i];
            bd[i] = take ? acc[i][j] : bd[i];
            bc[i] = take ? c : bc[i];
          }
        }
      });

  int nch = 0;
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    double d = bd[i];
    // a lane that saw no finite distance offers its smallest column at +inf (tx, when that is a
    // centroid): a row without any finite distance ends at c = 0
    int c = (bc[i] == INT_MAX && tx < K) ? tx : bc[i];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {   // stays inside the row's 16 lanes
      const double od = __shfl_xor(d, o);
      const int oc = __shfl_xor(c, o);
      const bool take = (od < d) | ((od == d) & (oc < c));
      d = take ? od : d;
      c = take ? oc : c;
    }
    const int qi = q0 + ty + 16 * i;
    const bool mine = tx == 0 && qi < nq;
    bool ch = false;
    if (mine) {
      const int q = qrow(qi);
      if (d == INFINITY) d = exact_dist(X + (int64_t)q * A, Cn + (int64_t)c * A, A);
      label[q] = c;
      dmin[q] = d;
      ch = prev != nullptr && prev[q] != c;
    }
    nch += __popcll(__ballot(ch));   // every lane of the wave reaches the ballot
  }
  if (changed != nullptr && nch != 0 && lane_id() == 0) atomicAdd(changed, nch);
}

}  // namespace dmlp
