// kmeans_screen.hip — the screened way to dmlp_kmeans_assign's answer (dmlp.h: k-means, screened):
// a single-term bf16 MFMA screen leaves a few candidate centroids per row, their exact fp64
// distances decide.  The same label, dmin and changed as k_kmeans_assign, bit for bit.
//
// Arithmetic.  Rows and centroids are centred on one mu (dmlp_center's rule over the rows; any mu
// is correct, it only tightens the bound).  With x' = x - mu, c' = c - mu and
// hi(v) = bf16(fp32(v)), the fp32 score of row i against centroid c is
//     a_ic = <hi(x_i'), hi(c')> - |c'|^2 / 2        (v_mfma_f32_16x16x32_bf16, C = -|c'|^2 / 2),
// an approximation of t_ic = <x_i', c'> - |c'|^2 / 2 = (|x_i'|^2 - d(x_i, c)) / 2: the largest t
// is the smallest distance.  dmlp_screen_x1_bound2(A, 2) bounds its error (screen_x1.hip):
//     |a_ic - t_ic| <= e_i = r1 |x_i'| M + r2 M^2,     M = max_c |c'|.
// The exact kernels do not minimise the real d but its fp64 evaluation D (each subtraction,
// product and sum rounded): |D - d| <= g d with g = (A + 2) 2^-53 (three roundings per term, A - 1
// per sum of non-negative terms).  If c* minimises D then d_c* (1 - g) <= d_c (1 + g) for every c,
// so t_c* >= t_c - g max(d) and max(d) <= (|x_i'| + M)^2.  Hence, with m_i = max_c a_ic,
//     a_ic* >= t_c* - e_i >= t_c - e_i - g max(d) >= a_c - 2 e_i - g max(d)   for every c,
// and the same holds for every centroid tied with c* in D.  The x1.25 that bound2 puts on r1 and
// r2 above the fp32 accumulation is what absorbs g max(d) in the k-NN screens, where |x'| and M
// are of one size (g <= 2^-46 against r1 / 4 >= 2^-10); here a row may lie far outside the
// centroids, so the term is carried explicitly: eps_i = e_i + r4 (|x_i'| + M)^2 + floor, r4 =
// 1.25 (A + 2) 2^-52, floor = 2^-100 (1 + |x_i'| + M) for operands and partial sums below the
// fp32 normal range.  Both additions only widen the keep rule
//     c is a candidate of row i  iff  a_ic >= m_i - 2 eps_i,
// which therefore keeps the exact winner and all its ties; a superset of candidates never changes
// the result, because the winner is chosen among them by the exact distance.
//
// Operands.  Rows: hi(x') as the MFMA B fragments, [row][kt][kg] 16-byte words (row's attributes
// 32 kt + 8 kg .. + 7), and |x'|^2 in fp32, made ONCE per fit (k_kmeans_rows; dmlp_prep_queries'
// rounding, but no lo half, KT = 3 without a pad to 4, and a row outside the screen's range —
// non-finite, or |x'| component >= 1e15 — is marked by a norm of +inf).  Centroids: prep.hip's
// tile image by dmlp_prep_data every call (K rows): hi fragments in A-operand order, -|c'|^2 / 2
// (-inf for the pad centroids of the last 64-tile), the rounded-up max norm, and *bad for a
// centroid outside the range.
//
// k_kmeans_screen<KT>: a workgroup is 4 waves, a wave owns 64 rows as four 16-row blocks whose
//   fragments stay in registers (16 KT VGPRs).  The centroid image goes through LDS in tiles of TS
//   16-centroid steps (TS KT KiB of fragments + 64 TS bytes of C operands) shared by the four
//   waves; a tile is fetched into registers while the previous one computes.  An image of one
//   tile (K <= 16 TS) is staged once for both passes.  Per step a wave reads KT fragments and one
//   C vector from LDS and issues 4 KT MFMAs.  Lane (c = lane & 15, kg = lane >> 4) then holds the
//   scores of row c of each block against centroids 4 kg .. 4 kg + 3 of the step.
//   Pass 1: one running maximum per accumulator register, then the maximum over the four
//   registers and the four kg lanes of the row: m_i.
//   Pass 2: the same MFMAs again; a score >= m_i - 2 eps_i appends its centroid to the row's list
//   (16 slots, global workspace).  Its slot is the row's count so far plus the hits of smaller
//   centroids in this step, taken from four ballots (one per accumulator register) masked to the
//   row's lanes: the list is in ascending c without an ordering race or an atomic.
//   End: count > 16, count == 0 (a NaN threshold), a marked row, or *bad: the row is escalated —
//   its count word is -1 and its id goes to the escalation list, placed by a ballot rank behind
//   one integer atomic per wave on stats[0].  stats[1] += the candidates of the other rows, one
//   atomic per workgroup.
// k_kmeans_pick: 64 rows per workgroup, 16 lanes per row, lane s takes candidate s: dmlp::exact_dist, then the
//   lexicographic (d, c) minimum over the 16 lanes — the contract's strict < in ascending c.  (A
//   screened row and all centroids are finite and below 1e15, so are its distances.)
// k_kmeans_escalate<PJ>: kmeans_tile.h over the listed rows; the grid is sized for N rows and a
//   workgroup past the device-side count returns at once.
// No host sync, no floating-point atomics; every loop is bounded by K or by the list capacity.
#include "dmlp.h"
#include "kmeans_tile.h"
#include <float.h>
#include <type_traits>

namespace {

constexpr int kMaxA = 128;           // KT <= 4
constexpr int kSlots = 16;           // candidate slots per row
constexpr int kMuBytes = 1024;       // the row handle's head: mu [A <= 128] doubles
constexpr double kMaxAbs = 1.0e15;   // prep.hip's range of |v - mu|

__host__ __device__ constexpr int screen_steps(int KT) { return KT == 1 ? 32 : KT == 2 ? 16 : 8; }

int64_t up256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// the per-call workspace
struct Ws {
  unsigned* words;   // [0] max |c'|^2 (fp32 bits, rounded up), [1] bad
  float* cinit;      // [Kpad]
  u32x4* cfrag;      // prep.hip's hi/lo tile image of the centroids
  int* cnt;          // [N] candidates of a row, -1: escalated
  int* esc;          // [N] escalated row ids, stats[0] of them
  int* cand;         // [N][kSlots]
  int64_t bytes;
};
Ws carve(void* ws, int64_t N, int KT, int K) {
  const int64_t kpad = ((int64_t)K + 63) / 64 * 64;
  char* p = (char*)ws;
  Ws w;
  int64_t o = 0;
  w.words = (unsigned*)(p + o); o += 256;
  w.cinit = (float*)(p + o); o += up256(kpad * 4);
  w.cfrag = (u32x4*)(p + o); o += up256(kpad * KT * 128);
  w.cnt = (int*)(p + o); o += up256(N * 4);
  w.esc = (int*)(p + o); o += up256(N * 4);
  w.cand = (int*)(p + o); o += up256(N * kSlots * 4);
  w.bytes = o;
  return w;
}

__global__ void k_screen_zero(unsigned* words, int* stats, int* changed) {
  words[0] = words[1] = 0u;
  stats[0] = stats[1] = 0;
  if (changed) *changed = 0;
}

// One thread per (row, 8-attribute group); a row's GP lanes (4 KT of them live) are adjacent, so
// |x'|^2 is a GP-lane xor-shuffle sum.
template <int KT>
__global__ __launch_bounds__(256) void k_kmeans_rows(const double* __restrict__ X, int64_t N,
                                                     int A, const double* __restrict__ mu,
                                                     uint4* __restrict__ xhi,
                                                     float* __restrict__ xn) {
  constexpr int GP = KT == 1 ? 4 : KT == 2 ? 8 : 16;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = gid / GP;
  const int g = (int)(gid - row * GP);
  const bool live = row < N && g < 4 * KT;
  unsigned short h[8];
  bool bad = false;
  double ss = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int a = g * 8 + j;
    double c = 0.0;
    if (live && a < A) {
      c = X[row * A + a] - mu[a];
      if (!(fabs(c) < kMaxAbs)) { bad = true; c = 0.0; }
    }
    ss += c * c;
    h[j] = __builtin_bit_cast(unsigned short, (__bf16)(float)c);   // round to nearest even
  }
  int nbad = bad;
#pragma unroll
  for (int o = 1; o < GP; o <<= 1) {
    ss += __shfl_xor(ss, o);
    nbad |= __shfl_xor(nbad, o);
  }
  if (!live) return;
  uint4 v;
  v.x = h[0] | ((unsigned)h[1] << 16); v.y = h[2] | ((unsigned)h[3] << 16);
  v.z = h[4] | ((unsigned)h[5] << 16); v.w = h[6] | ((unsigned)h[7] << 16);
  xhi[row * (4 * KT) + g] = v;
  if (g == 0) xn[row] = nbad ? INFINITY : (float)ss;
}

template <int KT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_kmeans_screen(
    const u32x4* __restrict__ xhi, const float* __restrict__ xn, int N,
    const u32x4* __restrict__ cfrag, const f32x4* __restrict__ cinit4, int K,
    const unsigned* __restrict__ words, float r1, float r2, float r4, int* __restrict__ cand,
    int* __restrict__ cnt_out, int* __restrict__ esc, int* __restrict__ stats) {
  constexpr int TS = screen_steps(KT);
  constexpr int NF = TS * KT * 64;   // 16-byte fragment words per tile
  constexpr int PF = NF / 256;       // of them per thread
  static_assert(NF % 256 == 0 && TS * 4 <= 256, "a tile is staged by whole workgroup passes");
  __shared__ u32x4 Fs[NF];
  __shared__ f32x4 Cs[TS * 4];

  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, kg = lane >> 4;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + (tid >> 6)) * 64;
  const int nsteps = ((K + 63) / 64) * 4;                // the image's 16-centroid steps
  const int ntile = (nsteps + TS - 1) / TS;
  const bool cbad = words[1] != 0u;                      // (workgroup-uniform)

  // ---- this wave's rows: fragments, eps, validity
  bf16x8 xb[4][KT];
  float eps[4];
  bool valid[4], rbad[4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
    const int64_t row = row0 + rb * 16 + c;
    valid[rb] = row < N;
    const int64_t rl = valid[rb] ? row : N - 1;   // (pads read the last row; never written)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
      xb[rb][kt] = __builtin_bit_cast(bf16x8, xhi[(rl * KT + kt) * 4 + kg]);
    const float q = xn[rl];
    rbad[rb] = !(q < INFINITY);
    const float cm = __uint_as_float(words[0]), sq = sqrtf(rbad[rb] ? 0.0f : q), sm = sqrtf(cm);
    eps[rb] = r1 * sq * sm + r2 * cm + r4 * (sq + sm) * (sq + sm) + 0x1p-100f * (1.0f + sq + sm);
  }

  int cnt[4] = {0, 0, 0, 0};
  if (!cbad) {
    // ---- staging: tile t's fragments and C operands, global -> registers -> LDS
    u32x4 fr[PF];
    f32x4 cr;
    auto fetch = [&](int t) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int e = tid + 256 * u, sk = e >> 6;   // sk = step-in-tile * KT + kt
        const bool in = t * TS + sk / KT < nsteps;
        fr[u] = in ? cfrag[((int64_t)t * (TS * KT) + sk) * 128 + (e & 63)] : u32x4{0u, 0u, 0u, 0u};
      }
      const bool in = tid < TS * 4 && t * TS + (tid >> 2) < nsteps;
      cr = in ? cinit4[(int64_t)t * (TS * 4) + tid]
              : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    };
    // it = 0 .. 2 ntile - 1: both passes' tiles in order; an image of one tile is staged once
    auto stage = [&](int it) __attribute__((always_inline)) {
      if (ntile == 1 && it > 0) return;
      __syncthreads();   // the previous tile's reads are done
#pragma unroll
      for (int u = 0; u < PF; ++u) Fs[tid + 256 * u] = fr[u];
      if (tid < TS * 4) Cs[tid] = cr;
      __syncthreads();
      if (ntile > 1 && it + 1 < 2 * ntile) fetch(it + 1 < ntile ? it + 1 : it + 1 - ntile);
    };

    float mx[4][4], thr[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx[rb][r] = -INFINITY;
    const unsigned long long rowm = 0x0001000100010001ull << c;   // the lanes holding row c
    const unsigned long long lowm = rowm & dmlp::lanemask_lt();   // of them, those of smaller kg

    auto pass = [&](auto P) __attribute__((always_inline)) {
      constexpr bool APPEND = decltype(P)::value;
      for (int t = 0; t < ntile; ++t) {
        stage(APPEND ? ntile + t : t);
        const int ns = nsteps - t * TS < TS ? nsteps - t * TS : TS;
        for (int s = 0; s < ns; ++s) {
          bf16x8 a[KT];
#pragma unroll
          for (int kt = 0; kt < KT; ++kt)
            a[kt] = __builtin_bit_cast(bf16x8, Fs[(s * KT + kt) * 64 + lane]);
          const f32x4 ci = Cs[s * 4 + kg];
          const int c0 = (t * TS + s) * 16 + kg * 4;   // this lane's first centroid of the step
#pragma unroll
          for (int rb = 0; rb < 4; ++rb) {
            f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], xb[rb][0], ci, 0, 0, 0);
#pragma unroll
            for (int kt = 1; kt < KT; ++kt)
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kt], xb[rb][kt], acc, 0, 0, 0);
            if constexpr (!APPEND) {
#pragma unroll
              for (int r = 0; r < 4; ++r) mx[rb][r] = fmaxf(mx[rb][r], acc[r]);
            } else {
              bool h[4];
#pragma unroll
              for (int r = 0; r < 4; ++r) h[r] = valid[rb] && acc[r] >= thr[rb];
              if (__ballot(h[0] | h[1] | h[2] | h[3]) != 0ull) {   // (wave-uniform)
                int slot = cnt[rb], total = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const unsigned long long b = __ballot(h[r]);
                  slot += __popcll(b & lowm);
                  total += __popcll(b & rowm);
                }
                int* const list = cand + (row0 + rb * 16 + c) * kSlots;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  if (h[r]) {
                    if (slot < kSlots) list[slot] = c0 + r;
                    ++slot;
                  }
                }
                cnt[rb] += total;
              }
            }
          }
        }
      }
    };

    fetch(0);
    pass(std::false_type{});
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      float m = fmaxf(fmaxf(mx[rb][0], mx[rb][1]), fmaxf(mx[rb][2], mx[rb][3]));
      m = fmaxf(m, __shfl_xor(m, 16));
      m = fmaxf(m, __shfl_xor(m, 32));
      thr[rb] = m - 2.0f * eps[rb];
    }
    pass(std::true_type{});
  }

  // ---- counts, the escalation list, stats (every lane of the wave reaches the ballots)
  unsigned long long em[4];
  int kept = 0, nesc = 0;
  bool e[4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
    const bool own = kg == 0 && valid[rb];
    e[rb] = own && (cbad || rbad[rb] || cnt[rb] > kSlots || cnt[rb] == 0);
    em[rb] = __ballot(e[rb]);
    nesc += __popcll(em[rb]);
    if (own) cnt_out[row0 + rb * 16 + c] = e[rb] ? -1 : cnt[rb];
    kept += own && !e[rb] ? cnt[rb] : 0;
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) kept += __shfl_xor(kept, o);   // (lanes >= 16 hold 0)
  int base = 0;
  if (lane == 0 && nesc) base = atomicAdd(&stats[0], nesc);
  base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
    if (e[rb]) esc[base + __popcll(em[rb] & dmlp::lanemask_lt())] = (int)(row0 + rb * 16 + c);
    base += __popcll(em[rb]);
  }
  // the candidate count: one atomic per workgroup (Cs is free: the passes are over)
  __syncthreads();
  int* const wk = (int*)Cs;
  if (lane == 0) wk[tid >> 6] = kept;
  __syncthreads();
  if (tid == 0 && wk[0] + wk[1] + wk[2] + wk[3] != 0)
    atomicAdd(&stats[1], wk[0] + wk[1] + wk[2] + wk[3]);
}

constexpr int kPickRows = 64;   // rows per workgroup of k_kmeans_pick, 16 at a time

__global__ __launch_bounds__(256) void k_kmeans_pick(
    const double* __restrict__ X, int N, int A, const double* __restrict__ Cn, int K,
    const int* __restrict__ cnt, const int* __restrict__ cand, const int* __restrict__ prev,
    int* __restrict__ label, double* __restrict__ dmin, int* changed) {
  __shared__ int wch[4];
  const int tid = threadIdx.x, s = tid & 15;
  int nch = 0;
#pragma unroll
  for (int i = 0; i < kPickRows / 16; ++i) {
    const int64_t row = (int64_t)blockIdx.x * kPickRows + i * 16 + (tid >> 4);
    const int n = row < N ? cnt[row] : -1;   // (-1: escalated, k_kmeans_escalate writes the row)
    double d = INFINITY;
    int c = INT_MAX;
    if (s < n) c = cand[row * kSlots + s];
    if ((unsigned)c < (unsigned)K) {   // (a listed id is a centroid; anything else is never read)
      const double v = dmlp::exact_dist(X + row * A, Cn + (int64_t)c * A, A);
      d = v != v ? INFINITY : v;   // (the contract's rank of a NaN; none arises here)
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {   // stays inside the row's 16 lanes
      const double od = __shfl_xor(d, o);
      const int oc = __shfl_xor(c, o);
      const bool take = (od < d) | ((od == d) & (oc < c));
      d = take ? od : d;
      c = take ? oc : c;
    }
    bool ch = false;
    if (s == 0 && n > 0) {
      label[row] = c;
      dmin[row] = d;
      ch = prev != nullptr && prev[row] != c;
    }
    nch += __popcll(__ballot(ch));
  }
  // one integer atomic per workgroup: same-address atomics serialise, and a first iteration
  // changes nearly every row
  if (dmlp::lane_id() == 0) wch[tid >> 6] = nch;
  __syncthreads();
  if (tid == 0) {
    const int t = wch[0] + wch[1] + wch[2] + wch[3];
    if (changed != nullptr && t != 0) atomicAdd(changed, t);
  }
}

template <int PJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PJ == 1 ? 4 : 2))) void
k_kmeans_escalate(const double* __restrict__ X, int A, const double* __restrict__ Cn, int K,
                  const int* __restrict__ prev, int* __restrict__ label,
                  double* __restrict__ dmin, int* changed, const int* __restrict__ list,
                  const int* __restrict__ count) {
  const int nq = *count, q0 = blockIdx.x * 64;
  if (q0 >= nq) return;   // (workgroup-uniform)
  dmlp::kmeans_assign_tile<PJ>(X, A, Cn, K, prev, label, dmin, changed, q0, nq,
                               [&](int qi) { return list[qi]; });
}

bool screen_shape_ok(int64_t N, int A, int64_t K) {
  return N >= 0 && N <= INT_MAX && A >= 1 && A <= kMaxA && K >= 0 && K <= INT_MAX - 128;
}

}  // namespace

extern "C" int dmlp_kmeans_screen_tile(int A) {
  return A >= 1 && A <= kMaxA ? 16 * screen_steps((A + 31) / 32) : -1;
}

extern "C" int64_t dmlp_kmeans_screen_rows_bytes(int64_t N, int A) {
  if (!screen_shape_ok(N, A, 0)) return -1;
  const int KT = (A + 31) / 32;
  return kMuBytes + up256(N * KT * 64) + up256(N * 4);
}

extern "C" int64_t dmlp_kmeans_screen_bytes(int64_t N, int A, int K) {
  if (!screen_shape_ok(N, A, K)) return -1;
  return carve(nullptr, N, (A + 31) / 32, K).bytes;
}

extern "C" int dmlp_kmeans_screen_layout(int64_t N, int A, int K, int64_t rows_off[2],
                                         int64_t ws_off[3]) {
  if (!screen_shape_ok(N, A, K) || !rows_off || !ws_off) return -1;
  const int KT = (A + 31) / 32;
  const Ws w = carve(nullptr, N, KT, K);
  rows_off[0] = kMuBytes;
  rows_off[1] = kMuBytes + up256(N * KT * 64);
  const char* const base = (const char*)w.words;   // (carve puts words at offset 0)
  ws_off[0] = (const char*)w.cnt - base;
  ws_off[1] = (const char*)w.esc - base;
  ws_off[2] = (const char*)w.cand - base;
  return 0;
}

extern "C" int dmlp_kmeans_screen_prep_rows(const double* X, int64_t N, int A, void* rows,
                                            int64_t rows_bytes, void* stream) {
  if (N == 0) return 0;
  if (!screen_shape_ok(N, A, 0) || !X || !rows ||
      rows_bytes < dmlp_kmeans_screen_rows_bytes(N, A))
    return -1;
  const int KT = (A + 31) / 32;
  hipStream_t st = (hipStream_t)stream;
  double* mu = (double*)rows;
  uint4* xhi = (uint4*)((char*)rows + kMuBytes);
  float* xn = (float*)((char*)xhi + up256(N * KT * 64));
  const int rc = dmlp_center(X, N, A, mu, stream);
  if (rc) return rc;
  const int gp = KT == 1 ? 4 : KT == 2 ? 8 : 16;
  const dim3 grid((unsigned)((N * gp + 255) / 256));
#define DMLP_KM_ROWS(KTV) \
  hipLaunchKernelGGL(k_kmeans_rows<KTV>, grid, dim3(256), 0, st, X, N, A, mu, xhi, xn)
  if (KT == 1) DMLP_KM_ROWS(1);
  else if (KT == 2) DMLP_KM_ROWS(2);
  else if (KT == 3) DMLP_KM_ROWS(3);
  else DMLP_KM_ROWS(4);
#undef DMLP_KM_ROWS
  DMLP_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmlp_kmeans_assign_screened(const void* rows, int64_t rows_bytes, const double* X,
                                           int64_t N, int A, const double* C, int K,
                                           const int* prev, int* label, double* dmin,
                                           int* changed, int* stats, void* ws, int64_t ws_bytes,
                                           void* stream) {
  if (N <= 0 || K <= 0) return 0;
  if (!screen_shape_ok(N, A, K) || !rows || !X || !C || !label || !dmin || !stats || !ws ||
      (changed && !prev) || rows_bytes < dmlp_kmeans_screen_rows_bytes(N, A) ||
      ws_bytes < dmlp_kmeans_screen_bytes(N, A, K))
    return -1;
  const int KT = (A + 31) / 32;
  const Ws w = carve(ws, N, KT, K);
  hipStream_t st = (hipStream_t)stream;
  const double* mu = (const double*)rows;
  const u32x4* xhi = (const u32x4*)((const char*)rows + kMuBytes);
  const float* xn = (const float*)((const char*)xhi + up256(N * KT * 64));

  hipLaunchKernelGGL(k_screen_zero, dim3(1), dim3(1), 0, st, w.words, stats, changed);
  DMLP_LAUNCH_CHECK();
  const int rc = dmlp_prep_data(C, K, A, mu, KT, w.cfrag, w.cinit, &w.words[0], &w.words[1], stream);
  if (rc) return rc;
  float r1, r2, r3;
  dmlp_screen_x1_bound2(A, 2, &r1, &r2, &r3);
  const float r4 = (float)(1.25 * (A + 2) * 0x1p-52);
  const dim3 sgrid((unsigned)((N + 255) / 256));
#define DMLP_KM_SCREEN(KTV)                                                                   \
  hipLaunchKernelGGL(k_kmeans_screen<KTV>, sgrid, dim3(256), 0, st, xhi, xn, (int)N, w.cfrag, \
                     (const f32x4*)w.cinit, K, w.words, r1, r2, r4, w.cand, w.cnt, w.esc, stats)
  if (KT == 1) DMLP_KM_SCREEN(1);
  else if (KT == 2) DMLP_KM_SCREEN(2);
  else if (KT == 3) DMLP_KM_SCREEN(3);
  else DMLP_KM_SCREEN(4);
#undef DMLP_KM_SCREEN
  DMLP_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_kmeans_pick, dim3((unsigned)((N + kPickRows - 1) / kPickRows)), dim3(256), 0, st, X, (int)N,
                     A, C, K, w.cnt, w.cand, prev, label, dmin, changed);
  DMLP_LAUNCH_CHECK();
  const dim3 egrid((unsigned)((N + 63) / 64));
  if (K <= dmlp::kAssignNarrowK)
    hipLaunchKernelGGL(k_kmeans_escalate<1>, egrid, dim3(256), 0, st, X, A, C, K, prev, label,
                       dmin, changed, w.esc, stats);
  else
    hipLaunchKernelGGL(k_kmeans_escalate<8>, egrid, dim3(256), 0, st, X, A, C, K, prev, label,
                       dmin, changed, w.esc, stats);
  DMLP_LAUNCH_CHECK();
  return 0;
}
