// vote_scores.hip — per-class vote counts and weighted votes of a neighbour list (dmlp.h: class
// scores): what predict_proba and the weighted predict read.
//
// A class's score is a sum of fp64 weights in LIST order (dmlp.h), so the classes are dealt to the
// lanes, not the entries: lane L owns class L + 64 * pass and walks the kept entries of the list
// front to back, adding 1 and w where the entry's class is its own.  The entries reach every lane
// by broadcast reads of a per-wave LDS strip.
//
// One wave per query row, rows taken grid-stride.  A list is taken in chunks of 256 slots, lane L
// holding slots L, L + 64, L + 128, L + 192 of a chunk (four groups of 64 consecutive slots, so a
// list of k <= 64 fills one group and the other three cost nothing): ballot / popcount compaction of the kept entries (the
// row's own id, padding and labels outside the class range dropped) into the strip as (class,
// weight) pairs, 3 KiB per wave, then the walk.  Mode 1 needs to know whether a kept entry of the
// row sits at d == 0 before the first weight is formed.
//   n <= 256 (one chunk: every search class but the exact path's k > 256): the list is loaded and
//     compacted once; the d == 0 ballot reads the registers, every class pass walks the same strip.
//   n > 256: mode 1 ballots d == 0 in a pass of its own over the list; then the class pass is the
//     outer loop and the list is read again per pass (a few KiB from L2), counts and sums staying
//     in registers over its chunks — not 64 passes of accumulators per lane.
// The winner is the largest (score bits, count, class) of the classes with a count — scores are
// >= 0, so their bit patterns order as integers — by a lane-local max over the passes and a 6-step
// wave reduction.
#include "dmlp.h"
#include "dmlp_device.h"

#include <algorithm>

namespace {

constexpr int kScoreChunk = 256;  // slots per chunk = 4 groups x 64 lanes
constexpr int kScoreWaves = 4;
constexpr int kScoreBlocks = 2048;
constexpr int kScoreCmax = 4096;

struct Row {  // what a wave knows about its row
  const double* d;
  const int* ids;
  const int* labels;
  int64_t in0;
  int n, sk, label_lo, nclass;
};

// One chunk of a list: which of this lane's four slots of [c0, min(c0 + 256, n)) are kept, their
// class (label - label_lo) and, in MODE 1, their distance (loaded beside the id, not behind the
// label it does not depend on).
template <int MODE>
__device__ __forceinline__ void load_chunk(const Row& r, int c0, int lane, bool (&kept)[4],
                                           int (&cls)[4], double (&dd)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    kept[i] = false;
    cls[i] = -1;
    dd[i] = 1.0;
    if (c0 + 64 * i < r.n) {  // (wave-uniform: a short list costs one group, not four)
      const int e = c0 + 64 * i + lane;  // (n <= kstride: e < n stays inside the row)
      const int id = e < r.n ? r.ids[r.in0 + e] : -1;
      if (MODE == 1 && e < r.n) dd[i] = r.d[r.in0 + e];
      bool k = id >= 0 && id != r.sk;
      const long long c = k ? (long long)r.labels[id] - (long long)r.label_lo : -1ll;
      k = k && c >= 0 && c < r.nclass;
      kept[i] = k;
      cls[i] = (int)c;
    }
  }
}

template <int MODE>
__device__ __forceinline__ bool chunk_has_zero(const bool (&kept)[4], const double (&dd)[4]) {
  bool z = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) z |= kept[i] && dd[i] == 0.0;
  return __ballot(z) != 0ull;
}

// The kept entries of a loaded chunk, in list order, into the strip as (class, weight); returns
// their number.  `zero`: the row's weight rule (dmlp.h).
template <int MODE>
__device__ __forceinline__ int compact_chunk(const bool (&kept)[4], const int (&cls)[4],
                                             const double (&dd)[4], bool zero, int lane, int* scls,
                                             double* sw) {
  const unsigned long long lt = dmlp::lanemask_lt();
  unsigned long long b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) b[i] = __ballot(kept[i]);
  dmlp::wave_sync();  // the walks of the strip's last content come first
  int M = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (b[i]) {  // (wave-uniform: no division for a group without a kept entry)
      const int pos = M + __popcll(b[i] & lt);  // (slot order: group i, then lane; pos <= 255)
      if (kept[i]) {
        scls[pos] = cls[i];
        if (MODE == 1) sw[pos] = zero ? (dd[i] == 0.0 ? 1.0 : 0.0) : 1.0 / dd[i];
      }
      M += __popcll(b[i]);
    }
  }
  // the walk reads classes four at a time: no class in the slots up to the next multiple of four
  if (lane < 3 && M + lane < kScoreChunk) scls[M + lane] = -1;
  dmlp::wave_sync();
  return M;
}

// Adds the strip's M entries of class `mine` to (cnt, sum), front to back.
template <int MODE>
__device__ __forceinline__ void walk_strip(const int* scls, const double* sw, int M, int mine,
                                           int& cnt, double& sum) {
  const int4* c4 = reinterpret_cast<const int4*>(scls);
  for (int t = 0; 4 * t < M; ++t) {
    const int4 c = c4[t];  // one address for the wave: a broadcast read
    cnt += (int)(c.x == mine) + (int)(c.y == mine) + (int)(c.z == mine) + (int)(c.w == mine);
    if (MODE == 1) {
      // (weights of the slots past M are stale: their class -1 never selects them)
      const double2 w01 = *reinterpret_cast<const double2*>(sw + 4 * t);
      const double2 w23 = *reinterpret_cast<const double2*>(sw + 4 * t + 2);
      sum = c.x == mine ? __dadd_rn(sum, w01.x) : sum;
      sum = c.y == mine ? __dadd_rn(sum, w01.y) : sum;
      sum = c.z == mine ? __dadd_rn(sum, w23.x) : sum;
      sum = c.w == mine ? __dadd_rn(sum, w23.y) : sum;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_vote_scores(
    const double* __restrict__ d, const int* __restrict__ ids, int kstride,
    const int* __restrict__ qk, int nq, const int* __restrict__ skip,
    const int* __restrict__ labels, int label_lo, int nclass, int* __restrict__ out_count,
    double* __restrict__ out_score, int* __restrict__ out_label) {
  __shared__ __attribute__((aligned(16))) int s_cls[kScoreWaves][kScoreChunk];
  __shared__ __attribute__((aligned(16))) double s_w[kScoreWaves][kScoreChunk];
  const int lane = dmlp::lane_id(), wave = threadIdx.x >> 6;
  int* scls = s_cls[wave];
  double* sw = s_w[wave];
  const int npass = (nclass + 63) >> 6;
  for (int64_t q = (int64_t)blockIdx.x * kScoreWaves + wave; q < nq;
       q += (int64_t)gridDim.x * kScoreWaves) {
    Row r;
    r.d = d, r.ids = ids, r.labels = labels;
    r.in0 = q * kstride;
    r.n = min(qk[q], kstride);     // (a negative k reads nothing)
    r.sk = skip ? skip[q] : -1;    // (kept ids are >= 0: -1 excludes nothing)
    r.label_lo = label_lo, r.nclass = nclass;
    const int64_t out0 = q * nclass;
    const bool single = r.n <= kScoreChunk;  // (wave-uniform)
    bool kept[4];
    int cls[4];
    double dd[4];
    bool zero = false;
    int M = 0;
    if (single) {
      load_chunk<MODE>(r, 0, lane, kept, cls, dd);
      if (MODE == 1) zero = chunk_has_zero<MODE>(kept, dd);
      M = compact_chunk<MODE>(kept, cls, dd, zero, lane, scls, sw);
    } else if (MODE == 1) {
      for (int c0 = 0; c0 < r.n; c0 += kScoreChunk) {
        load_chunk<MODE>(r, c0, lane, kept, cls, dd);
        zero |= chunk_has_zero<MODE>(kept, dd);
      }
    }
    long long best_s = -1ll, best_k = -1ll;  // score bits; (count << 32) | class
    for (int pass = 0; pass < npass; ++pass) {
      const int mine = (pass << 6) + lane;
      int cnt = 0;
      double sum = 0.0;
      if (single) {
        walk_strip<MODE>(scls, sw, M, mine, cnt, sum);
      } else {
        for (int c0 = 0; c0 < r.n; c0 += kScoreChunk) {
          load_chunk<MODE>(r, c0, lane, kept, cls, dd);
          M = compact_chunk<MODE>(kept, cls, dd, zero, lane, scls, sw);
          walk_strip<MODE>(scls, sw, M, mine, cnt, sum);
        }
      }
      if (MODE == 0) sum = (double)cnt;
      if (mine < nclass) {
        if (out_count) out_count[out0 + mine] = cnt;
        if (out_score) out_score[out0 + mine] = sum;
        if (cnt > 0) {
          const long long s = __double_as_longlong(sum);
          const long long k = ((long long)cnt << 32) | (long long)mine;
          if (s > best_s || (s == best_s && k > best_k)) {
            best_s = s;
            best_k = k;
          }
        }
      }
    }
    if (out_label) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const long long os = __shfl_xor(best_s, off), ok = __shfl_xor(best_k, off);
        if (os > best_s || (os == best_s && ok > best_k)) {
          best_s = os;
          best_k = ok;
        }
      }
      if (lane == 0)
        out_label[q] = best_k < 0 ? -1 : (int)((long long)label_lo + (best_k & 0xffffffffll));
    }
  }
}

}  // namespace

extern "C" int dmlp_vote_scores_cmax(void) { return kScoreCmax; }

extern "C" int dmlp_vote_scores(const double* d, const int* ids, int kstride, const int* qk, int nq,
                                const int* skip, const int* labels, int label_lo, int nclass,
                                int mode, int* out_count, double* out_score, int* out_label,
                                void* stream) {
  if (nq <= 0) return 0;
  if (nclass < 1 || nclass > kScoreCmax || kstride < 1 || mode < 0 || mode > 1) return -1;
  if ((mode == 1 && !d) || (!out_count && !out_score && !out_label)) return -1;
  if (!ids || !qk || !labels) return -1;
  const int blocks = std::min((nq - 1) / kScoreWaves + 1, kScoreBlocks);
  auto kern = mode == 1 ? k_vote_scores<1> : k_vote_scores<0>;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(64 * kScoreWaves), 0, (hipStream_t)stream, d, ids,
                     kstride, qk, nq, skip, labels, label_lo, nclass, out_count, out_score,
                     out_label);
  DMLP_LAUNCH_CHECK();
  return 0;
}
