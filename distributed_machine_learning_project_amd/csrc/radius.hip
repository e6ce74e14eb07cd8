// radius.hip — fixed-radius search: every point n with d(q, x_n) <= r2[q] (r2 a SQUARED radius, one
// fp64 per query, the boundary inclusive), d the reference's fp64 distance (engine.cpp:12-18: left
// to right over the attributes, each subtraction, product and sum separately rounded — no FMA).
//
// Two passes over the distance tile k_exact_topk uses (fp64_tile.h: 64 queries x 128 points per
// workgroup) with none of its selection: no candidate buffers, no moving threshold, no
// compaction.  A query's 16 threads sit in ONE wave, so both passes are deterministic without LDS
// buffers and without atomics:
//   count  every lane counts its own hits per row; one 16-lane reduction at the end.
//   fill   the same distances again; per offer round (one point column j, points p0 + tx + 16 j)
//          and row one full-wave ballot of the hit predicate: a lane's rank is the popcount of its
//          query's 16-bit field below its tx, and every lane of the 16 advances the row's running
//          total by the field's popcount.  Points arrive in ascending id, so slot off + count - 1 -
//          (total + rank) gives DESCENDING id with no ordering race.
// dmlp_radius_sort then orders each segment by distance with the stable segmented radix sort
// fallback.hip uses: stability on descending-id input is (dist asc, id desc) without a composite
// key.
#include <hipcub/hipcub.hpp>

#include "dmlp.h"
#include "fp64_tile.h"
#include <limits.h>
#include <math.h>

namespace {

// exact.hip's ExK16 tile without the buffers: 64 queries x 128 points, 16 attributes per chunk
using Rd = dmlp::Fp64Tile<64, 8, 16>;

template <bool FILL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_radius(
    const double* __restrict__ X, int64_t N, int A, const double* __restrict__ Qx, int nq,
    const double* __restrict__ r2, const int* __restrict__ count, const int64_t* __restrict__ off,
    int* __restrict__ out_count, double* __restrict__ out_d, int* __restrict__ out_i) {
  constexpr int QB = Rd::QB, PJ = Rd::PJ, PT = Rd::PT, AS = Rd::AS, RI = Rd::RI;
  __shared__ __attribute__((aligned(16))) double Qs[QB][AS];
  __shared__ __attribute__((aligned(16))) double Xs[PT][AS];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int q0 = blockIdx.x * QB;
  // this thread's rows: ty + 16 i.  A pad query (q >= nq) gets a NaN radius, which no distance
  // is <= to: it neither counts nor writes, whatever the r2 of the real rows.
  double rq[RI];
  int hits[RI];        // count: this lane's hits; fill: slots of the segment still free (uniform
                       // over the row's 16 lanes)
  int64_t base[RI];
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    const int q = q0 + ty + 16 * i;
    rq[i] = q < nq ? r2[q] : NAN;
    hits[i] = 0;
    base[i] = 0;
    if (FILL && q < nq) {
      hits[i] = count[q];
      base[i] = off[q];
    }
  }
  const unsigned below = (1u << tx) - 1u;       // the row's lanes before this one
  const int fshift = ((tid & 63) >> 4) << 4;    // the row's 16-bit field of a ballot

  dmlp::fp64_tile_scan<Rd>(
      X, N, A, Qx, q0, nq, Qs, Xs, [](int qi) { return qi; },
      [&](int64_t p0, const double (&acc)[RI][PJ]) __attribute__((always_inline)) {
        // offer the tile's distances, one point column per round (<= 16 per query per round);
        // pad points of the last tile (p >= N) are no hits, with r2 = +inf too
#pragma unroll
        for (int j = 0; j < PJ; ++j) {
          const int64_t p = p0 + tx + 16 * j;
#pragma unroll
          for (int i = 0; i < RI; ++i) {
            const bool hit = p < N && acc[i][j] <= rq[i];
            if (!FILL) {
              hits[i] += hit ? 1 : 0;
            } else {
              // every lane of the wave reaches the ballot: it stands outside the divergent write
              const unsigned field = (unsigned)(__ballot(hit) >> fshift) & 0xffffu;
              const int slot = hits[i] - 1 - __popc(field & below);
              if (hit && slot >= 0) {  // a hit past the segment's count is dropped, never written
                out_d[base[i] + slot] = acc[i][j];
                out_i[base[i] + slot] = (int)p;
              }
              hits[i] -= __popc(field);
            }
          }
        }
      });
  if (!FILL) {
#pragma unroll
    for (int i = 0; i < RI; ++i) {
      int c = hits[i];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) c += __shfl_xor(c, o);   // stays inside the row's 16 lanes
      const int q = q0 + ty + 16 * i;
      if (tx == 0 && q < nq) out_count[q] = c;
    }
  }
}

// One wave per segment: its 32-bit begin / end offsets for the segmented sort, and its entries
// copied to the workspace (the sort reads them there and writes the caller's arrays).  A segment
// that is empty, starts below 0 or reaches past cap (the span the workspace was sized for) is given
// to the sort as empty and stays as it is.
__global__ __launch_bounds__(64) void k_radius_stage(const double* __restrict__ d,
                                                     const int* __restrict__ ids,
                                                     const int* __restrict__ count,
                                                     const int64_t* __restrict__ off, int nq,
                                                     int64_t cap, double* __restrict__ td,
                                                     int* __restrict__ ti, int* __restrict__ beg,
                                                     int* __restrict__ end) {
  const int q = blockIdx.x;
  if (q >= nq) return;
  const int64_t o = off[q];
  int c = count[q];
  if (c <= 0 || o < 0 || o > cap - c) c = 0;
  if (threadIdx.x == 0) {
    beg[q] = c ? (int)o : 0;
    end[q] = c ? (int)(o + c) : 0;
  }
  for (int j = threadIdx.x; j < c; j += 64) {
    td[o + j] = d[o + j];
    ti[o + j] = ids[o + j];
  }
}

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

size_t sort_temp_bytes(int64_t span, int nq) {
  size_t bytes = 0;
  hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, bytes, (const double*)nullptr,
                                              (double*)nullptr, (const int*)nullptr, (int*)nullptr,
                                              (int)span, nq, (const int*)nullptr,
                                              (const int*)nullptr);
  return bytes;
}

int64_t sort_bytes(int64_t span, int nq) {
  return (int64_t)(align_up((size_t)span * 8) + align_up((size_t)span * 4) +
                   2 * align_up((size_t)nq * 4) + align_up(sort_temp_bytes(span, nq)));
}

int radius_args(const double* X, int64_t N, int A, const double* Qx, const double* r2) {
  if (N > INT_MAX || A < 1 || !Qx || !r2 || (N > 0 && !X)) return -1;
  return 0;
}

}  // namespace

extern "C" int dmlp_radius_count(const double* X, int64_t N, int A, const double* Qx, int nq,
                                 const double* r2, int* out_count, void* stream) {
  if (nq <= 0) return 0;
  if (radius_args(X, N, A, Qx, r2) || !out_count) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (N <= 0) {
    const hipError_t e = hipMemsetAsync(out_count, 0, (size_t)nq * sizeof(int), st);
    return e == hipSuccess ? 0 : -(int)e;
  }
  hipLaunchKernelGGL(k_radius<false>, dim3((unsigned)((nq + Rd::QB - 1) / Rd::QB)), dim3(256), 0,
                     st, X, N, A, Qx, nq, r2, (const int*)nullptr, (const int64_t*)nullptr,
                     out_count, (double*)nullptr, (int*)nullptr);
  DMLP_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmlp_radius_fill(const double* X, int64_t N, int A, const double* Qx, int nq,
                                const double* r2, const int* count, const int64_t* off,
                                double* out_d, int* out_i, void* stream) {
  if (nq <= 0) return 0;
  if (radius_args(X, N, A, Qx, r2) || !count || !off || !out_d || !out_i) return -1;
  if (N <= 0) return 0;
  hipLaunchKernelGGL(k_radius<true>, dim3((unsigned)((nq + Rd::QB - 1) / Rd::QB)), dim3(256), 0,
                     (hipStream_t)stream, X, N, A, Qx, nq, r2, count, off, (int*)nullptr, out_d,
                     out_i);
  DMLP_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t dmlp_radius_sort_bytes(int64_t span, int nq) {
  if (span < 0 || span > INT_MAX || nq < 0) return -1;
  return sort_bytes(span, nq);
}

extern "C" int dmlp_radius_sort(double* d, int* ids, const int* count, const int64_t* off, int nq,
                                void* ws, int64_t ws_bytes, void* stream) {
  if (nq <= 0) return 0;
  if (!d || !ids || !count || !off || !ws) return -1;
  // The span this workspace was sized for: the largest one whose advertised size fits.  (The
  // segments live on the device, so their span is the caller's statement, made through ws_bytes.)
  if (ws_bytes < sort_bytes(0, nq)) return -1;
  int64_t cap = 0, hi = INT_MAX;
  while (cap < hi) {
    const int64_t mid = cap + (hi - cap + 1) / 2;
    if (sort_bytes(mid, nq) <= ws_bytes) cap = mid; else hi = mid - 1;
  }
  if (cap == 0) return 0;   // room for empty segments only: nothing to sort
  hipStream_t st = (hipStream_t)stream;
  char* p = (char*)ws;
  double* td = (double*)p; p += align_up((size_t)cap * 8);
  int* ti = (int*)p; p += align_up((size_t)cap * 4);
  int* beg = (int*)p; p += align_up((size_t)nq * 4);
  int* end = (int*)p; p += align_up((size_t)nq * 4);
  size_t tmp_bytes = sort_temp_bytes(cap, nq);
  hipLaunchKernelGGL(k_radius_stage, dim3((unsigned)nq), dim3(64), 0, st, d, ids, count, off, nq,
                     cap, td, ti, beg, end);
  DMLP_LAUNCH_CHECK();
  // non-negative doubles order like their bit patterns; stable LSD radix keeps id-desc ties
  const hipError_t e = hipcub::DeviceSegmentedRadixSort::SortPairs(
      p, tmp_bytes, td, d, ti, ids, (int)cap, nq, beg, end, 0, 64, st);
  return e == hipSuccess ? 0 : -(int)e;
}
