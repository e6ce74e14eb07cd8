// vote_curve.hip — the vote of every prefix of a sorted neighbour list (dmlp.h: vote curve and
// weighted vote curve): one kernel template, k_vote_curve<MODE>.
//
// The lists come out of the search sorted by (dist asc, id desc), so the vote for every k <= kmax
// is a function of ONE list.  For kept entry e let c_e = #{kept e' <= e with e's label} and
// key_e = (c_e << 32) | (label_e ^ 0x80000000), wave_vote_by's key: the largest key over a prefix
// names its vote (max count, ties -> larger label), because the running count of the winning
// label is reached by exactly one entry of the prefix.  The curve is an inclusive prefix max of
// the keys — no label histogram, so any int is a label.
//
// MODE 1 (weighted): with s_e the running score of e's class — the sum, in list order from 0.0, of
// the weights of the kept e' <= e with e's label — the key grows to (s_e, c_e, label_e): weights
// are >= 0, so a class's (s, c) never decreases along the list, and the largest key over a prefix
// is the largest (score, count, label) over its classes, dmlp_vote_scores' rule.  MODE 0 (uniform)
// forms no weight: its score is (double)count, so (s, c, label) orders exactly like (c, label) and
// the one-word key serves; the score column, where asked for, is the key's count.
//
// One wave per query row, lane L holding slots 4L .. 4L + 3: ballot / popcount compaction of the
// kept entries (the row's own id and padding dropped), labels (MODE 1: and weights) staged in a
// 1 KiB (2 KiB) LDS strip per wave, counts by broadcast reads of that strip — MODE 1 adds a
// matching earlier-or-equal entry's weight beside the count, entries ascending, so every sum is
// left to right —, the prefix max as an in-lane scan plus a 6-step cross-lane scan.  Rows are taken
// grid-stride, so the per-k hit counts stay in registers over a wave's rows, meet in LDS once per
// workgroup and reach memory as one atomicAdd per k.
#include "dmlp.h"
#include "dmlp_device.h"

#include <math.h>

#include <algorithm>

namespace {

constexpr int kCurveMax = 256;  // slots per row = 64 lanes x 4 = the workgroup's threads
constexpr int kCurveWaves = 4;
constexpr int kCurveBlocks = 2048;

// The scanned key of an entry: k = (count << 32) | (label ^ 0x80000000), in MODE 1 behind the
// score's bits (scores are >= 0, so their bits order as integers).  Negative: no entry.
template <int MODE>
struct CurveKey;

template <>
struct CurveKey<0> {
  long long k;
  __device__ __forceinline__ static CurveKey make(double, long long k) { return {k}; }
  __device__ __forceinline__ static CurveKey empty() { return {-1ll}; }
  __device__ __forceinline__ CurveKey max(CurveKey o) const { return k > o.k ? *this : o; }
  __device__ __forceinline__ CurveKey shfl_up(int o) const { return {__shfl_up(k, o)}; }
  __device__ __forceinline__ double score() const { return (double)(k >> 32); }
};

template <>
struct CurveKey<1> {
  long long s, k;
  __device__ __forceinline__ static CurveKey make(double s, long long k) {
    return {__double_as_longlong(s), k};
  }
  __device__ __forceinline__ static CurveKey empty() { return {-1ll, -1ll}; }
  __device__ __forceinline__ CurveKey max(CurveKey o) const {
    return (s > o.s || (s == o.s && k > o.k)) ? *this : o;
  }
  __device__ __forceinline__ CurveKey shfl_up(int o) const {
    return {__shfl_up(s, o), __shfl_up(k, o)};
  }
  __device__ __forceinline__ double score() const { return __longlong_as_double(s); }
};

template <int MODE>
__global__ __launch_bounds__(256) void k_vote_curve(
    const double* __restrict__ d, const int* __restrict__ ids, int kstride,
    const int* __restrict__ qk, int nq, const int* __restrict__ skip,
    const int* __restrict__ labels, int kcap, int* __restrict__ out_label,
    double* __restrict__ out_score, double* __restrict__ out_d, int* __restrict__ out_i,
    const int* __restrict__ truth, unsigned long long* __restrict__ hits) {
  using Key = CurveKey<MODE>;
  __shared__ __attribute__((aligned(16))) int s_lab[kCurveWaves][kCurveMax];
  __shared__ int s_hits[kCurveMax];
  const int lane = dmlp::lane_id(), wave = threadIdx.x >> 6;
  if (hits) {
    s_hits[threadIdx.x] = 0;
    __syncthreads();
  }
  int* strip = s_lab[wave];
  double* sw = nullptr;  // MODE 1: the weights beside the labels
  if constexpr (MODE == 1) {
    __shared__ __attribute__((aligned(16))) double s_w[kCurveWaves][kCurveMax];
    sw = s_w[wave];
  }
  const unsigned long long lt = dmlp::lanemask_lt();
  int hacc[4] = {0, 0, 0, 0};
  for (int64_t q = (int64_t)blockIdx.x * kCurveWaves + wave; q < nq;
       q += (int64_t)gridDim.x * kCurveWaves) {
    const int n = min(min(qk[q], kstride), kCurveMax);  // (a negative k reads nothing)
    const int sk = skip ? skip[q] : -1;                 // (kept ids are >= 0: -1 excludes nothing)
    const int64_t in0 = q * kstride, out0 = q * kcap;
    int id[4], lb[4];
    double dd[4];
    bool kept[4];
    unsigned long long b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = 4 * lane + i;
      id[i] = e < n ? ids[in0 + e] : -1;
      dd[i] = 1.0;
      if (MODE == 1 && e < n) dd[i] = d[in0 + e];  // (beside the id, not behind the label)
      kept[i] = id[i] >= 0 && id[i] != sk;
      lb[i] = kept[i] ? labels[id[i]] : 0;
      b[i] = __ballot(kept[i]);
    }
    int pos = 0, M = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pos += __popcll(b[i] & lt);
      M += __popcll(b[i]);
    }
    const int m = min(M, kcap);
    // the row's weight rule, from its first kept entry: the first lane that keeps one, and that
    // lane's first kept slot
    bool zero = false;
    if (MODE == 1) {
      const unsigned long long anyb = b[0] | b[1] | b[2] | b[3];
      const double mine = kept[0] ? dd[0] : kept[1] ? dd[1] : kept[2] ? dd[2] : dd[3];
      const int fl = anyb ? __builtin_ctzll(anyb) : 0;
      const double d0 = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(mine), fl),
                                         __builtin_amdgcn_readlane(__double2loint(mine), fl));
      zero = anyb != 0ull && d0 == 0.0;
    }
    dmlp::wave_sync();  // the last row's strip reads come first
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (kept[i]) {
        strip[pos] = lb[i];  // (pos <= 255)
        if (MODE == 1) sw[pos] = zero ? (dd[i] == 0.0 ? 1.0 : 0.0) : 1.0 / dd[i];
        if (out_i && pos < kcap) {
          out_i[out0 + pos] = id[i];
          out_d[out0 + pos] = MODE == 1 ? dd[i] : d[in0 + 4 * lane + i];
        }
        ++pos;
      }
    }
    if (out_i) {
      for (int j = m + lane; j < kcap; j += 64) {
        out_i[out0 + j] = -1;
        out_d[out0 + j] = INFINITY;
      }
    }
    dmlp::wave_sync();
    // the compacted list: lane L now holds kept entries 4L .. 4L + 3
    int cl[4], c[4];
    double s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      cl[i] = 4 * lane + i < M ? strip[4 * lane + i] : 0;
      c[i] = 0;
      s[i] = 0.0;
    }
    const int4* s4 = reinterpret_cast<const int4*>(strip);
    for (int t = 0; 4 * t < M; ++t) {
      const int4 v = s4[t];  // one address for the wave: a broadcast read
      const int r = 4 * lane - 4 * t;  // entry j' = 4t + u counts for j = 4L + i when u <= r + i
      // (slots of the strip past M hold stale labels and weights: they pair only with j >= M,
      // whose key is dropped below)
      double2 w01, w23;
      if (MODE == 1) {
        w01 = *reinterpret_cast<const double2*>(sw + 4 * t);
        w23 = *reinterpret_cast<const double2*>(sw + 4 * t + 2);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool hx = (v.x == cl[i]) & (0 <= r + i), hy = (v.y == cl[i]) & (1 <= r + i),
                   hz = (v.z == cl[i]) & (2 <= r + i), hw = (v.w == cl[i]) & (3 <= r + i);
        c[i] += (int)hx + (int)hy + (int)hz + (int)hw;
        if (MODE == 1) {
          s[i] = hx ? __dadd_rn(s[i], w01.x) : s[i];
          s[i] = hy ? __dadd_rn(s[i], w01.y) : s[i];
          s[i] = hz ? __dadd_rn(s[i], w23.x) : s[i];
          s[i] = hw ? __dadd_rn(s[i], w23.y) : s[i];
        }
      }
    }
    Key key[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      key[i] = 4 * lane + i < M
                   ? Key::make(s[i], ((long long)c[i] << 32) |
                                         (long long)((unsigned)cl[i] ^ 0x80000000u))
                   : Key::empty();
      if (i) key[i] = key[i].max(key[i - 1]);
    }
    Key incl = key[3];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const Key t = incl.shfl_up(o);
      if (lane >= o) incl = incl.max(t);
    }
    Key excl = incl.shfl_up(1);
    if (lane == 0) excl = Key::empty();
    const int tr = truth ? truth[q] : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * lane + i;
      if (j < kcap) {
        // slots past the kept entries carry the last prefix's key on: label and score repeat, and
        // a row without a kept entry holds (-1, 0.0) throughout
        const Key kj = key[i].max(excl);
        const int lab = kj.k < 0 ? -1 : (int)((unsigned)(kj.k & 0xffffffffll) ^ 0x80000000u);
        out_label[out0 + j] = lab;
        if (out_score) out_score[out0 + j] = kj.k < 0 ? 0.0 : kj.score();
        hacc[i] += (int)(truth != nullptr && lab == tr);
      }
    }
  }
  if (hits) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (hacc[i]) atomicAdd(&s_hits[4 * lane + i], hacc[i]);
    __syncthreads();
    const int cnt = s_hits[threadIdx.x];
    if ((int)threadIdx.x < kcap && cnt) atomicAdd(&hits[threadIdx.x], (unsigned long long)cnt);
  }
}

int launch_curve(const double* d, const int* ids, int kstride, const int* qk, int nq,
                 const int* skip, const int* labels, int mode, int kcap, int* out_label,
                 double* out_score, double* out_d, int* out_i, const int* truth,
                 unsigned long long* hits, void* stream) {
  if (nq <= 0) return 0;
  if (kcap < 1 || kcap > kCurveMax || kstride < 1 || mode < 0 || mode > 1) return -1;
  if ((out_d == nullptr) != (out_i == nullptr) || (truth == nullptr) != (hits == nullptr))
    return -1;
  if (!ids || !qk || !labels || !out_label || ((out_d || mode == 1) && !d)) return -1;
  const int blocks = std::min((nq - 1) / kCurveWaves + 1, kCurveBlocks);
  auto kern = mode == 1 ? k_vote_curve<1> : k_vote_curve<0>;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(64 * kCurveWaves), 0, (hipStream_t)stream, d, ids,
                     kstride, qk, nq, skip, labels, kcap, out_label, out_score, out_d, out_i, truth,
                     hits);
  DMLP_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dmlp_vote_curve_kmax(void) { return kCurveMax; }

extern "C" int dmlp_vote_curve(const double* d, const int* ids, int kstride, const int* qk, int nq,
                               const int* skip, const int* labels, int kcap, int* out_label,
                               double* out_d, int* out_i, const int* truth,
                               unsigned long long* hits, void* stream) {
  return launch_curve(d, ids, kstride, qk, nq, skip, labels, 0, kcap, out_label, nullptr, out_d,
                      out_i, truth, hits, stream);
}

extern "C" int dmlp_vote_curve_weighted(const double* d, const int* ids, int kstride, const int* qk,
                                        int nq, const int* skip, const int* labels, int mode,
                                        int kcap, int* out_label, double* out_score, double* out_d,
                                        int* out_i, const int* truth, unsigned long long* hits,
                                        void* stream) {
  return launch_curve(d, ids, kstride, qk, nq, skip, labels, mode, kcap, out_label, out_score,
                      out_d, out_i, truth, hits, stream);
}
