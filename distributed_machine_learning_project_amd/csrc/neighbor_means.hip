// neighbor_means.hip — the (weighted) mean of the targets of a neighbour list, and of every prefix
// of it (dmlp.h: neighbour means): what KNNRegressor's predict, predict_curve and leave-one-out
// curves read.
//
// One wave per query row, rows taken grid-stride.  A list is taken in chunks of 256 slots, lane L
// holding slots L, L + 64, L + 128, L + 192 of a chunk (a list of k <= 64 fills one group, the
// other three cost nothing): ballot / popcount compaction of the kept entries (the row's own id and
// padding dropped) into a per-wave LDS strip in list order, then a walk of the strip front to back.
// Mode 1 weighs by d_ref / d, d_ref the distance of the row's FIRST kept entry: it is fetched from
// the lane that holds it (the lowest set bit of the first non-empty ballot) before the first weight
// is formed, and kept over the chunks of a long list, as the sums are.
//
// A mean is sum_t / wsum, both fp64 sums in LIST order (dmlp.h): only the __dadd_rn chains are
// serial, so everything else is taken off them.
//   T >= 2 (k_neighbor_means): the targets are dealt to the lanes, not the entries: lane L owns
//     target column L + 64 * pass (T <= 256: at most four sums per lane, all in registers).  The
//     strip holds (id, weight) pairs, 3 KiB per wave; an entry's id is wave-uniform, so its gather
//     is one coalesced run of 8 T bytes.  The walk takes four entries at a time: their gathers and
//     products do not depend on the running sums, so all of them are issued before the first add.
//       whole list: every chunk of [0, min(k, kstride)), one division per target at the end.
//       curve: one chunk (256 slots at most), sum / wsum stored after every kept entry of the same
//         walk, which stops at kcap entries; the slots behind the last one repeat it (staged in
//         the strip, then written as one contiguous run).
//   T == 1 (k_neighbor_means_t1): dealing one column to 64 lanes would leave one lane gathering
//     four targets at a time.  The gather rides on the compaction instead: every lane fetches the
//     target of its own entries (up to 256 loads in flight per wave) and stores the rounded product
//     w * y, and w, into the strip (4 KiB per wave in mode 1, 2 KiB in mode 0); the walk is two
//     add chains over broadcast reads.  In the curve lane j % 64 keeps the running (sum, wsum)
//     after entry j, and the divisions and the stores of a row are done by all lanes at once.
//     Same operations in the same order as the general form: the same bits.
#include "dmlp.h"
#include "dmlp_device.h"

#include <math.h>

#include <algorithm>

namespace {

constexpr int kMeanChunk = 256;  // slots per chunk = 4 groups x 64 lanes
constexpr int kMeanWaves = 4;
constexpr int kMeanBlocks = 2048;
constexpr int kMeanTmax = 256;   // 4 passes of 64 lanes
constexpr int kMeanPass = kMeanTmax / 64;

__device__ __forceinline__ double quiet_nan() {
  return __longlong_as_double(0x7ff8000000000000ll);
}

// dmlp.h's weight of an entry at distance x in a row whose first kept entry sits at dref
__device__ __forceinline__ double weight_of(double dref, double x) {
  if (dref == 0.0) return x == 0.0 ? 1.0 : 0.0;
  if (dref == INFINITY) return 1.0;
  return __ddiv_rn(dref, x);
}

struct Row {  // what a wave knows about its row
  const double* d;
  const int* ids;
  int64_t in0;
  int n, sk;
  double dref;  // mode 1: the distance of the first kept entry, once `have`
  bool have;
};

struct Chunk {  // this lane's four slots of a chunk
  int id[4];
  double dd[4];
  bool kept[4];
  unsigned long long b[4];  // the wave's ballots of kept[i]
};

// One chunk of a list: which of this lane's four slots of [c0, min(c0 + 256, n)) are kept and, in
// MODE 1, their distance; the row's d_ref when this chunk holds its first kept entry.
template <int MODE>
__device__ __forceinline__ void load_chunk(Row& r, int c0, int lane, Chunk& c) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c.id[i] = -1;
    c.dd[i] = 1.0;
    if (c0 + 64 * i < r.n) {  // (wave-uniform: a short list costs one group, not four)
      const int e = c0 + 64 * i + lane;  // (n <= kstride: e < n stays inside the row)
      if (e < r.n) {
        c.id[i] = r.ids[r.in0 + e];
        if (MODE == 1) c.dd[i] = r.d[r.in0 + e];
      }
    }
    c.kept[i] = c.id[i] >= 0 && c.id[i] != r.sk;
    c.b[i] = __ballot(c.kept[i]);
  }
  if (MODE == 1 && !r.have) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!r.have && c.b[i]) {  // (wave-uniform)
        r.dref = __shfl(c.dd[i], __ffsll((long long)c.b[i]) - 1);
        r.have = true;
      }
    }
  }
}

template <int MODE, bool CURVE>
__global__ __launch_bounds__(256) void k_neighbor_means(
    const double* __restrict__ d, const int* __restrict__ ids, int kstride,
    const int* __restrict__ qk, int nq, const int* __restrict__ skip,
    const double* __restrict__ targets, int T, int kcap, double* __restrict__ out_mean,
    double* __restrict__ out_wsum, int* __restrict__ out_count) {
  __shared__ __attribute__((aligned(16))) int s_id[kMeanWaves][kMeanChunk];
  __shared__ __attribute__((aligned(16))) double s_w[kMeanWaves][kMeanChunk];
  const int lane = dmlp::lane_id(), wave = threadIdx.x >> 6;
  int* sid = s_id[wave];
  double* sw = s_w[wave];
  const unsigned long long lt = dmlp::lanemask_lt();
  const int npass = (T + 63) >> 6;
  for (int64_t q = (int64_t)blockIdx.x * kMeanWaves + wave; q < nq;
       q += (int64_t)gridDim.x * kMeanWaves) {
    Row r;
    r.d = d, r.ids = ids;
    r.in0 = q * kstride;
    r.n = min(qk[q], kstride);  // (a negative k reads nothing)
    if (CURVE) r.n = min(r.n, kMeanChunk);
    r.sk = skip ? skip[q] : -1;  // (kept ids are >= 0: -1 excludes nothing)
    r.dref = 1.0, r.have = false;
    const int64_t out0 = CURVE ? q * kcap : q;  // rows of T means in front of this query's
    double sum[kMeanPass] = {0.0, 0.0, 0.0, 0.0};
    double wsum = 0.0;
    int m = 0;  // kept entries walked so far
    for (int c0 = 0; c0 < r.n; c0 += kMeanChunk) {
      Chunk c;
      load_chunk<MODE>(r, c0, lane, c);
      // ---- the kept entries, in list order, into the strip as (id, weight)
      dmlp::wave_sync();  // the walk of the strip's last content comes first
      int M = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (c.b[i]) {  // (wave-uniform: no division for a group without a kept entry)
          const int pos = M + __popcll(c.b[i] & lt);  // (slot order: group i, then lane; <= 255)
          if (c.kept[i]) {
            sid[pos] = c.id[i];
            if (MODE == 1) sw[pos] = weight_of(r.dref, c.dd[i]);
          }
          M += __popcll(c.b[i]);
        }
      }
      dmlp::wave_sync();
      if (CURVE) M = min(M, kcap);  // (one chunk: m == 0 here)
      // ---- the walk: four entries' gathers and products ahead of their adds
      for (int j0 = 0; j0 < M; j0 += 4) {
        const int4 e = *reinterpret_cast<const int4*>(sid + j0);  // one address: a broadcast read
        const bool on[4] = {true, j0 + 1 < M, j0 + 2 < M, j0 + 3 < M};  // (wave-uniform)
        // (slots past M hold stale ids: the first entry's row is fetched in their place)
        const int idu[4] = {e.x, on[1] ? e.y : e.x, on[2] ? e.z : e.x, on[3] ? e.w : e.x};
        double w[4] = {1.0, 1.0, 1.0, 1.0};
        if (MODE == 1) {
          const double2 w01 = *reinterpret_cast<const double2*>(sw + j0);
          const double2 w23 = *reinterpret_cast<const double2*>(sw + j0 + 2);
          w[0] = w01.x, w[1] = w01.y, w[2] = w23.x, w[3] = w23.y;
        }
        double v[4][kMeanPass];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double* row = targets + (int64_t)idu[u] * T;
#pragma unroll
          for (int p = 0; p < kMeanPass; ++p) {
            const int t = 64 * p + lane;
            v[u][p] = (p < npass && t < T) ? row[t] : 0.0;
            if (MODE == 1) v[u][p] = __dmul_rn(w[u], v[u][p]);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (on[u]) {
#pragma unroll
            for (int p = 0; p < kMeanPass; ++p) sum[p] = __dadd_rn(sum[p], v[u][p]);
            if (MODE == 1) wsum = __dadd_rn(wsum, w[u]);
            if (CURVE) {
              const int j = j0 + u;
              const double ws = MODE == 1 ? wsum : (double)(j + 1);
#pragma unroll
              for (int p = 0; p < kMeanPass; ++p) {
                const int t = 64 * p + lane;
                if (p < npass && t < T) out_mean[(out0 + j) * T + t] = __ddiv_rn(sum[p], ws);
              }
            }
          }
        }
      }
      m += M;
    }
    if (MODE == 0) wsum = (double)m;
    double last[kMeanPass];
#pragma unroll
    for (int p = 0; p < kMeanPass; ++p) last[p] = m ? __ddiv_rn(sum[p], wsum) : quiet_nan();
    if (!CURVE) {
#pragma unroll
      for (int p = 0; p < kMeanPass; ++p) {
        const int t = 64 * p + lane;
        if (p < npass && t < T) out_mean[out0 * T + t] = last[p];
      }
      if (lane == 0) {
        if (out_wsum) out_wsum[q] = wsum;  // (0.0 for a row that keeps nothing)
        if (out_count) out_count[q] = m;
      }
    } else if (m < kcap) {  // (wave-uniform) slots [m, kcap) repeat the last computed one
      dmlp::wave_sync();  // the walk's reads of the strip come first
#pragma unroll
      for (int p = 0; p < kMeanPass; ++p) {
        const int t = 64 * p + lane;
        if (p < npass && t < T) sw[t] = last[p];  // (T <= 256 = the strip)
      }
      dmlp::wave_sync();
      double* tail = out_mean + (out0 + m) * T;
      const int cnt = (kcap - m) * T;  // (<= 256 * 256)
      for (int x = lane; x < cnt; x += 64) tail[x] = sw[x % T];
    }
  }
}

// T == 1: the gather rides on the compaction (the file's head).
template <int MODE, bool CURVE>
__global__ __launch_bounds__(256) void k_neighbor_means_t1(
    const double* __restrict__ d, const int* __restrict__ ids, int kstride,
    const int* __restrict__ qk, int nq, const int* __restrict__ skip,
    const double* __restrict__ targets, int kcap, double* __restrict__ out_mean,
    double* __restrict__ out_wsum, int* __restrict__ out_count) {
  __shared__ __attribute__((aligned(16))) double s_p[kMeanWaves][kMeanChunk];
  __shared__ __attribute__((aligned(16))) double s_w[kMeanWaves][MODE == 1 ? kMeanChunk : 2];
  const int lane = dmlp::lane_id(), wave = threadIdx.x >> 6;
  double* sp = s_p[wave];
  double* sw = s_w[wave];
  const unsigned long long lt = dmlp::lanemask_lt();
  for (int64_t q = (int64_t)blockIdx.x * kMeanWaves + wave; q < nq;
       q += (int64_t)gridDim.x * kMeanWaves) {
    Row r;
    r.d = d, r.ids = ids;
    r.in0 = q * kstride;
    r.n = min(qk[q], kstride);  // (a negative k reads nothing)
    if (CURVE) r.n = min(r.n, kMeanChunk);
    r.sk = skip ? skip[q] : -1;  // (kept ids are >= 0: -1 excludes nothing)
    r.dref = 1.0, r.have = false;
    double sum = 0.0, wsum = 0.0;
    double ksum[4] = {0.0, 0.0, 0.0, 0.0}, kws[4] = {1.0, 1.0, 1.0, 1.0};  // after entry lane + 64 g
    int m = 0;
    for (int c0 = 0; c0 < r.n; c0 += kMeanChunk) {
      Chunk c;
      load_chunk<MODE>(r, c0, lane, c);
      double y[4];  // this lane's entries' targets: all of the wave's gathers in flight at once
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] = c.kept[i] ? targets[c.id[i]] : 0.0;
      // ---- the kept entries, in list order, into the strip as (product, weight)
      dmlp::wave_sync();  // the walk of the strip's last content comes first
      int M = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (c.b[i]) {  // (wave-uniform: no division for a group without a kept entry)
          const int pos = M + __popcll(c.b[i] & lt);  // (slot order: group i, then lane; <= 255)
          if (c.kept[i]) {
            if (MODE == 1) {
              const double w = weight_of(r.dref, c.dd[i]);
              sw[pos] = w;
              sp[pos] = __dmul_rn(w, y[i]);
            } else {
              sp[pos] = y[i];
            }
          }
          M += __popcll(c.b[i]);
        }
      }
      dmlp::wave_sync();
      if (CURVE) M = min(M, kcap);  // (one chunk: m == 0 here)
      // ---- the walk: the two add chains, every lane the same; group g holds entries 64 g ..
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        for (int j0 = 64 * g; j0 < min(M, 64 * g + 64); j0 += 4) {
          // (one address for the wave: broadcast reads; slots past M hold stale values)
          const double2 p01 = *reinterpret_cast<const double2*>(sp + j0);
          const double2 p23 = *reinterpret_cast<const double2*>(sp + j0 + 2);
          const double p[4] = {p01.x, p01.y, p23.x, p23.y};
          double w[4] = {1.0, 1.0, 1.0, 1.0};
          if (MODE == 1) {
            const double2 w01 = *reinterpret_cast<const double2*>(sw + j0);
            const double2 w23 = *reinterpret_cast<const double2*>(sw + j0 + 2);
            w[0] = w01.x, w[1] = w01.y, w[2] = w23.x, w[3] = w23.y;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (j0 + u < M) {  // (wave-uniform)
              sum = __dadd_rn(sum, p[u]);
              if (MODE == 1) wsum = __dadd_rn(wsum, w[u]);
              if (CURVE && ((j0 + u) & 63) == lane) {
                ksum[g] = sum;
                kws[g] = MODE == 1 ? wsum : (double)(j0 + u + 1);
              }
            }
          }
        }
      }
      m += M;
    }
    if (MODE == 0) wsum = (double)m;
    const double last = m ? __ddiv_rn(sum, wsum) : quiet_nan();
    if (!CURVE) {
      if (lane == 0) {
        out_mean[q] = last;
        if (out_wsum) out_wsum[q] = wsum;  // (0.0 for a row that keeps nothing)
        if (out_count) out_count[q] = m;
      }
    } else {
      // the row's divisions and stores by all lanes at once; slots [m, kcap) repeat the last one
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j = 64 * g + lane;
        if (j < kcap) out_mean[q * kcap + j] = j < m ? __ddiv_rn(ksum[g], kws[g]) : last;
      }
    }
  }
}

}  // namespace

extern "C" int dmlp_neighbor_means_tmax(void) { return kMeanTmax; }

static int launch_means(const double* d, const int* ids, int kstride, const int* qk, int nq,
                        const int* skip, const double* targets, int T, int mode, int kcap,
                        bool curve, double* out_mean, double* out_wsum, int* out_count,
                        void* stream) {
  if (nq <= 0) return 0;
  if (T < 1 || T > kMeanTmax || kstride < 1 || mode < 0 || mode > 1) return -1;
  if (curve && (kcap < 1 || kcap > kMeanChunk)) return -1;
  if ((mode == 1 && !d) || !out_mean || !ids || !qk || !targets) return -1;
  const int blocks = std::min((nq - 1) / kMeanWaves + 1, kMeanBlocks);
  if (T == 1) {
    auto kern = curve
                    ? (mode == 1 ? k_neighbor_means_t1<1, true> : k_neighbor_means_t1<0, true>)
                    : (mode == 1 ? k_neighbor_means_t1<1, false> : k_neighbor_means_t1<0, false>);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64 * kMeanWaves), 0, (hipStream_t)stream, d, ids,
                       kstride, qk, nq, skip, targets, kcap, out_mean, out_wsum, out_count);
  } else {
    auto kern = curve ? (mode == 1 ? k_neighbor_means<1, true> : k_neighbor_means<0, true>)
                      : (mode == 1 ? k_neighbor_means<1, false> : k_neighbor_means<0, false>);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64 * kMeanWaves), 0, (hipStream_t)stream, d, ids,
                       kstride, qk, nq, skip, targets, T, kcap, out_mean, out_wsum, out_count);
  }
  DMLP_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmlp_neighbor_means(const double* d, const int* ids, int kstride, const int* qk,
                                   int nq, const int* skip, const double* targets, int T, int mode,
                                   double* out_mean, double* out_wsum, int* out_count,
                                   void* stream) {
  return launch_means(d, ids, kstride, qk, nq, skip, targets, T, mode, 1, false, out_mean,
                      out_wsum, out_count, stream);
}

extern "C" int dmlp_neighbor_means_curve(const double* d, const int* ids, int kstride,
                                         const int* qk, int nq, const int* skip,
                                         const double* targets, int T, int mode, int kcap,
                                         double* out_mean, void* stream) {
  return launch_means(d, ids, kstride, qk, nq, skip, targets, T, mode, kcap, true, out_mean,
                      nullptr, nullptr, stream);
}
