// exact.hip — fused streaming exact top-k (k <= 256): fp64 distances in the reference's order
// (engine.cpp:12-18: left to right over the attributes, each subtraction, product and sum
// separately rounded — no FMA) and the per-query selection in ONE pass, with no Q x N distance
// rows in HBM (fallback.hip writes every row, then radix-selects it: ~5 HBM passes per row).
//
// The distances come from fp64_tile.h's tile (QB = 64 queries per workgroup; 16 for k > 64): a
// query's 16 threads all sit in ONE wave, so every query's candidate buffer is wave-private and
// needs no workgroup barrier.  After a tile, its distances are offered in PJ rounds (one point
// column j per round, <= 16 candidates per query): a distance is appended iff it is <= the query's
// current threshold T (the k-th best so far; points arrive in increasing id order, so a later
// point equal to T — larger id — ranks before it under (dist asc, id desc) and must be kept).
// Before a round, if some buffer of the wave could overflow, the wave compacts: every entry's
// rank among its query's buffer (key_less, exact order), the best k rewritten in sorted order,
// T = the k-th.  At the end one compaction sorts every buffer and the first k go out.
#include "dmlp.h"
#include "fp64_tile.h"
#include <math.h>
#include <stdlib.h>

namespace {

// The tile (fp64_tile.h: QB, PJ, AC) plus CB candidate slots per query.
template <int QB_, int PJ_, int CB_, int AC_, int WPE_ = 2>
struct Ex : dmlp::Fp64Tile<QB_, PJ_, AC_> {
  static constexpr int CB = CB_;
  static constexpr int WPE = WPE_;    // waves per SIMD the kernel is compiled for
  static constexpr int EPL = (CB + 63) / 64;  // buffer entries per lane in a compaction
  static constexpr int BUF = QB_ * CB * (8 + 4) + QB_ * 4 + QB_ * 8;   // entries + counts + T
  static constexpr int LDS = Ex::STG + BUF;
};
using ExK16 = Ex<64, 8, 48, 16>;    // k <= 16: 2 workgroups per CU
// (measured and dropped: a 4x4 micro-tile with 32-slot buffers at 3 waves per SIMD — 73.5 ms
// against 54.1 ms, profiles/r4l_exact_variants.txt: the extra LDS reads per fp64 op cost more
// than the occupancy hides)
using ExK32 = Ex<64, 8, 64, 16>;
using ExK64 = Ex<64, 8, 128, 16>;
using ExK256 = Ex<16, 16, 384, 8>;  // k <= 256: 16 queries per workgroup, 384-slot buffers

// The candidate buffers, behind the tile's staging in the workgroup's dynamic LDS.  They are taken
// from the LDS symbol where they are used, not passed down as pointers: compact_rows is compiled
// out of line, and only an address it can see to be 16-byte aligned LDS lets its rank loop unroll
// into b128 reads.
template <class C>
struct Bufs {
  double* bd;   // [QB][CB]
  int* bi;      // [QB][CB]
  int* cnt;     // [QB]
  double* thr;  // [QB]
  __device__ __forceinline__ Bufs() {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bd = (double*)(smem + C::STG);
    bi = (int*)(bd + C::QB * C::CB);
    cnt = bi + C::QB * C::CB;
    thr = (double*)(cnt + C::QB);
  }
};

// Compact every row of wave `wave` that holds more than its k entries (final: every row, and
// write the sorted first k out).  Rows of wave w: ty in [4w, 4w + 4) x i -> 4 RI rows.  Rare
// (a few times per query), so it is an out-of-line call: inlined at every offer round it
// would inflate the hot loop's register allocation.
template <class C>
__device__ __noinline__ void compact_rows(const int* __restrict__ qidx,
                                          const int* __restrict__ qk, int nb, int64_t N, int q0,
                                          int wave, int lane, bool final_pass,
                                          double* __restrict__ out_d, int* __restrict__ out_i,
                                          int kstride) {
  constexpr int CB = C::CB, EPL = C::EPL;
  const Bufs<C> b;
  double* __restrict__ const bd = b.bd;
  int* __restrict__ const bi = b.bi;
  int* __restrict__ const cnt = b.cnt;
  double* __restrict__ const thr = b.thr;
  for (int s = 0; s < 4 * C::RI; ++s) {
    const int r = (4 * wave + (s & 3)) + 16 * (s >> 2);
    const int n = cnt[r];
    const int q = q0 + r;
    int k = 0;
    if (q < nb) {
      k = qk[qidx[q]];
      if ((int64_t)k > N) k = (int)N;
    }
    if (!final_pass && n <= k) continue;
    double* rd = bd + r * CB;
    int* ri = bi + r * CB;
    // ranks of this lane's entries (lane + 64 h) under (dist asc, id desc)
    double ed[EPL];
    int ei[EPL], rk[EPL];
#pragma unroll
    for (int h = 0; h < EPL; ++h) {
      const int e = lane + 64 * h;
      rk[h] = 1 << 30;
      if (e < n) {
        ed[h] = rd[e];
        ei[h] = ri[e];
        int c = 0;
        for (int j = 0; j < n; ++j) c += dmlp::key_less(rd[j], ri[j], ed[h], ei[h]) ? 1 : 0;
        rk[h] = c;
      }
    }
    dmlp::wave_sync();  // every lane has read the buffer before any rewrite
    const int kept = n < k ? n : k;
#pragma unroll
    for (int h = 0; h < EPL; ++h) {
      if (rk[h] < kept) {
        if (final_pass) {
          out_d[(int64_t)qidx[q] * kstride + rk[h]] = ed[h];
          out_i[(int64_t)qidx[q] * kstride + rk[h]] = ei[h];
        } else {
          rd[rk[h]] = ed[h];
          ri[rk[h]] = ei[h];
        }
      }
    }
    dmlp::wave_sync();
    if (lane == 0) {
      cnt[r] = kept;
      thr[r] = (!final_pass && kept == k && k > 0) ? rd[k - 1] : INFINITY;
    }
    dmlp::wave_sync();
  }
}

template <class C>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(C::WPE))) void k_exact_topk(const double* __restrict__ X, int64_t N, int A,
                                                    const double* __restrict__ Qx,
                                                    const int* __restrict__ qidx,
                                                    const int* __restrict__ qk, int nb,
                                                    double* __restrict__ out_d,
                                                    int* __restrict__ out_i, int kstride) {
  constexpr int QB = C::QB, PJ = C::PJ, CB = C::CB, AS = C::AS, RI = C::RI;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double (*Qs)[AS] = (double (*)[AS])smem;
  double (*Xs)[AS] = (double (*)[AS])(smem + QB * AS * 8);
  const Bufs<C> b;
  double* const bd = b.bd;
  int* const bi = b.bi;
  int* const cnt = b.cnt;
  double* const thr = b.thr;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * QB;
  // this thread's rows: ty + 16 i; per-row k (0 for rows past nb)
  int kq[RI];
  double tq[RI];
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    const int r = ty + 16 * i;
    kq[i] = q0 + r < nb ? qk[qidx[q0 + r]] : 0;
    if ((int64_t)kq[i] > N) kq[i] = (int)N;
    tq[i] = INFINITY;
  }
  if (tid < QB) { cnt[tid] = 0; thr[tid] = INFINITY; }
  __syncthreads();

  dmlp::fp64_tile_scan<C>(
      X, N, A, Qx, q0, nb, Qs, Xs, [&](int qi) { return qidx[qi]; },
      [&](int64_t p0, const double (&acc)[RI][PJ]) __attribute__((always_inline)) {
        // offer the tile's distances, one point column per round (<= 16 per query per round)
#pragma unroll
        for (int j = 0; j < PJ; ++j) {
          bool full = false;
#pragma unroll
          for (int i = 0; i < RI; ++i) full |= cnt[ty + 16 * i] > CB - 16;
          if (__ballot(full)) {
            compact_rows<C>(qidx, qk, nb, N, q0, wave, lane, false, out_d, out_i, kstride);
#pragma unroll
            for (int i = 0; i < RI; ++i) tq[i] = thr[ty + 16 * i];
          }
          const int64_t p = p0 + tx + 16 * j;
#pragma unroll
          for (int i = 0; i < RI; ++i) {
            if (p < N && kq[i] > 0 && acc[i][j] <= tq[i]) {
              const int r = ty + 16 * i;
              const int pos = atomicAdd(&cnt[r], 1);
              bd[r * CB + pos] = acc[i][j];
              bi[r * CB + pos] = (int)p;
            }
          }
          dmlp::wave_sync();
        }
      });
  compact_rows<C>(qidx, qk, nb, N, q0, wave, lane, true, out_d, out_i, kstride);
}

template <class C>
int launch_exact(const double* X, int64_t N, int A, const double* Qx, const int* qidx,
                 const int* qk, int nb, double* out_d, int* out_i, int kstride, hipStream_t st) {
  const int lds = C::LDS;
  static const bool attr = hipFuncSetAttribute((const void*)&k_exact_topk<C>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               lds) == hipSuccess;
  if (!attr) return -5;
  hipLaunchKernelGGL((k_exact_topk<C>), dim3((unsigned)((nb + C::QB - 1) / C::QB)), dim3(256),
                     lds, st, X, N, A, Qx, qidx, qk, nb, out_d, out_i, kstride);
  DMLP_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dmlp_exact_topk_kmax(void) { return 256; }
// The largest k the fused kernel should take for a dataset of N points.  For k in (64, 256] its
// rank-based compactions of 384-slot buffers cost about as much as the distances when N is
// small (N = 1e5, k = 200: 93.6 ms vs 23.5 ms for rows + radix select), and win once the
// rows' HBM traffic grows (N = 1e6: 260 vs 756 ms; N = 1e7: 1.5 s vs > 170 s).
extern "C" int dmlp_exact_topk_kmax_for(int64_t N) { return N >= (int64_t(1) << 19) ? 256 : 64; }

// Exact top-k (k <= 256, clamped to N) of queries qidx[0..nb), sorted by (dist asc, id desc) into
// out_*[q * kstride + j], j < k (slots past min(k, N) untouched).  kmax: an upper bound of the
// k of these queries (selects the buffer size).  No workspace.
extern "C" int dmlp_exact_topk(const double* X, int64_t N, int A, const double* Qx,
                               const int* qidx, const int* qk, int nb, int kmax, double* out_d,
                               int* out_i, int kstride, void* stream) {
  if (nb <= 0 || N <= 0) return 0;
  if (N > 0x7fffffff || A < 1 || kmax > 256) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (kmax <= 16) return launch_exact<ExK16>(X, N, A, Qx, qidx, qk, nb, out_d, out_i, kstride, st);
  if (kmax <= 32) return launch_exact<ExK32>(X, N, A, Qx, qidx, qk, nb, out_d, out_i, kstride, st);
  if (kmax <= 64) return launch_exact<ExK64>(X, N, A, Qx, qidx, qk, nb, out_d, out_i, kstride, st);
  return launch_exact<ExK256>(X, N, A, Qx, qidx, qk, nb, out_d, out_i, kstride, st);
}
