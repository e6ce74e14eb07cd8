// fp64_tile.h — the fp64 distance tile of exact.hip (k_exact_topk) and radius.hip (k_radius):
// distances in the reference's order (engine.cpp:12-18: left to right over the attributes, each
// subtraction, product and sum separately rounded — no FMA) of QB queries against the whole data
// stream, with no Q x N distance rows in HBM.
//
// Workgroup = 256 threads = QB queries; the data stream is tiled by PT = 16 PJ points.  Thread
// (tx = tid & 15, ty = tid >> 4) owns the RI x PJ micro-tile (RI = QB / 16) of queries ty + 16 i
// and points tx + 16 j of the tile, so a query's 16 threads all sit in ONE wave.  The attributes
// are taken in chunks of AC, query and point chunks staged in LDS (rows of AS doubles).  The
// staging is software-pipelined: the next (tile, chunk)'s elements are loaded into registers while
// the current chunk computes, so no wave waits on global memory at the barriers.  After a tile's
// last chunk its distances acc[i][j] are handed to the kernel's `offer`.
#pragma once
#include "dmlp_device.h"

namespace dmlp {

// QB queries per workgroup, PJ points per thread per tile, AC attributes per LDS chunk.
template <int QB_, int PJ_, int AC_>
struct Fp64Tile {
  static constexpr int QB = QB_, PJ = PJ_, PT = 16 * PJ_, AC = AC_;
  static constexpr int AS = AC + 2;   // LDS row stride in doubles: 16-byte aligned rows (b128)
  static constexpr int RI = QB / 16;  // rows (queries) per thread
  static constexpr int NQ = (QB * AC + 255) / 256, NX = (PT * AC + 255) / 256;
  static constexpr int STG = (QB + PT) * AS * 8;  // Qs + Xs chunk staging
};

// Every tile of X[0..N) against query slots q0 .. q0 + QB (slots >= nq are pads: zeros).  Qs
// [QB][AS] and Xs [PT][AS] are the workgroup's staging; qrow(qi) is the row of Qx that slot qi
// reads; offer(p0, acc) takes the distances of points p0 + tx + 16 j (pads past N included) once
// per tile.  All 256 threads call it together (it holds workgroup barriers).
template <class C, class QRow, class Offer>
__device__ __forceinline__ void fp64_tile_scan(const double* __restrict__ X, int64_t N, int A,
                                               const double* __restrict__ Qx, int q0, int nq,
                                               double (*Qs)[C::AS], double (*Xs)[C::AS], QRow qrow,
                                               Offer offer) {
  constexpr int QB = C::QB, PJ = C::PJ, PT = C::PT, AC = C::AC;
  constexpr int RI = C::RI, NQ = C::NQ, NX = C::NX;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double qr[NQ], xr[NX];
  auto fetch = [&](int64_t p0, int a0) __attribute__((always_inline)) {
    const int ac = A - a0 < AC ? A - a0 : AC;
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      const int e = tid + 256 * u, r = e / AC, a = e % AC;
      const int qi = q0 + r;
      qr[u] = (e < QB * AC && qi < nq && a < ac) ? Qx[(int64_t)qrow(qi) * A + a0 + a] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < NX; ++u) {
      const int e = tid + 256 * u, r = e / AC, a = e % AC;
      const int64_t pi = p0 + r;
      xr[u] = (e < PT * AC && pi < N && a < ac) ? X[pi * A + a0 + a] : 0.0;
    }
  };
  fetch(0, 0);
  for (int64_t p0 = 0; p0 < N; p0 += PT) {
    double acc[RI][PJ];
#pragma unroll
    for (int i = 0; i < RI; ++i)
#pragma unroll
      for (int j = 0; j < PJ; ++j) acc[i][j] = 0.0;
    for (int a0 = 0; a0 < A; a0 += AC) {
      const int ac = A - a0 < AC ? A - a0 : AC;
      __syncthreads();  // the previous chunk's reads are done
#pragma unroll
      for (int u = 0; u < NQ; ++u)
        if (tid + 256 * u < QB * AC) Qs[(tid + 256 * u) / AC][(tid + 256 * u) % AC] = qr[u];
#pragma unroll
      for (int u = 0; u < NX; ++u)
        if (tid + 256 * u < PT * AC) Xs[(tid + 256 * u) / AC][(tid + 256 * u) % AC] = xr[u];
      __syncthreads();
      {
        int64_t np = p0;
        int na = a0 + AC;
        if (na >= A) { na = 0; np = p0 + PT; }
        if (np < N) fetch(np, na);
      }
      // two attributes per step: 16-byte LDS reads; the sums stay in attribute order
      int a = 0;
      for (; a + 1 < ac; a += 2) {
        double2 qv[RI], xv[PJ];
#pragma unroll
        for (int i = 0; i < RI; ++i) qv[i] = *(const double2*)&Qs[ty + 16 * i][a];
#pragma unroll
        for (int j = 0; j < PJ; ++j) xv[j] = *(const double2*)&Xs[tx + 16 * j][a];
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
          for (int j = 0; j < PJ; ++j) {
            const double d0 = __dsub_rn(qv[i].x, xv[j].x);
            acc[i][j] = __dadd_rn(acc[i][j], __dmul_rn(d0, d0));
            const double d1 = __dsub_rn(qv[i].y, xv[j].y);
            acc[i][j] = __dadd_rn(acc[i][j], __dmul_rn(d1, d1));
          }
      }
      if (a < ac) {  // odd attribute count: the last one alone
        double qv[RI], xv[PJ];
#pragma unroll
        for (int i = 0; i < RI; ++i) qv[i] = Qs[ty + 16 * i][a];
#pragma unroll
        for (int j = 0; j < PJ; ++j) xv[j] = Xs[tx + 16 * j][a];
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
          for (int j = 0; j < PJ; ++j) {
            const double d0 = __dsub_rn(qv[i], xv[j]);
            acc[i][j] = __dadd_rn(acc[i][j], __dmul_rn(d0, d0));
          }
      }
    }
    offer(p0, acc);
  }
}

}  // namespace dmlp
