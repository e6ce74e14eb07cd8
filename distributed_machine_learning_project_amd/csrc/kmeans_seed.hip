// kmeans_seed.hip — D^2 (k-means++) seeding on the device (dmlp.h: k-means seeding), bit-identical
// to dmlp_cpu_kmeans_seed: no FMA, no floating-point atomics, every sum in the contract's fixed
// order (rows in runs of 64, runs in blocks of 64, the blocks left to right).  The random numbers
// u come from the caller, so a seeding is 2K launches on one stream without a host sync.
//
//   k_seed_update   once per seed, the hot kernel: reads all of X once.  A wave owns one run of 64
//     rows, the lane is the row.  A lane walking its own row-major row would read with a stride of
//     A * 8 bytes; instead the wave stages its 64 x 16 tile through LDS: 16 coalesced loads of 64
//     doubles (four rows' 128-byte pieces each) into registers, written to LDS with a row stride
//     of 17 doubles — odd, so the 32 lanes of one ds_read_b64 pass, reading column a of 32
//     different rows, fall on 32 different bank pairs.  The next chunk's loads are issued before
//     the current chunk's arithmetic, and the lane carries its distance s across the chunks in
//     attribute order (any A).  A wave's stage is its own: no workgroup barrier, a workgroup is
//     four independent waves whose add chains hide under each other's loads.  The centre row is
//     wave-uniform and read through uniform loads.  Then w_i = d < w_i ? d : w_i, v_i = w_i < inf
//     ? w_i : 0, and the run sum R_r by the strict chain over the 64 lanes (lane broadcasts).
//   k_seed_pick     one workgroup per seed.  Its threads take the blocks in parallel, each summing
//     its 64 run sums in order (B_b); wave 0 then walks: 64 values per coalesced load, the running
//     sum chained over the lanes while every lane keeps the sum BEFORE its own term, so that
//     s + x > t is one compare per lane and the first hit a ballot.  Once over the blocks for T,
//     again for the block, then the block's runs, then the run's rows.  The workgroup writes
//     seeds[j] and copies the row into C[j], threads as columns.  Step 0 only copies row i0.
//
// A lane past the end of a short run (or a thread past the last run of a block) adds 0.0 to the
// chain: every sum here is >= +0.0 (v_i >= +0.0, never NaN), and s + 0.0 == s bit for bit for such
// s, so the short run's sum is the contract's.
#include "dmlp.h"
#include "dmlp_device.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int kWaves = 4;             // waves (runs) per workgroup of k_seed_update
constexpr int kChunk = 16;            // attributes per LDS stage
constexpr int kStride = kChunk + 1;   // doubles per staged row: odd
constexpr int kPickThreads = 256;
constexpr int kPickAhead = 16;        // run sums in flight ahead of a block's add chain

// lane L's x in every lane (L wave-uniform)
__device__ __forceinline__ double lane_bcast(double x, int L) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), L);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), L);
  return __hiloint2double(hi, lo);
}

// ((s + v_0) + v_1) + ... + v_63 over the lanes of a wave, one rounded add per lane in lane
// order; before = the sum as it stood before this lane's term
__device__ __forceinline__ double lane_chain(double s, double v, double& before) {
  const int lane = dmlp::lane_id();
#pragma unroll
  for (int L = 0; L < 64; ++L) {
    if (lane == L) before = s;
    s = __dadd_rn(s, lane_bcast(v, L));
  }
  return s;
}

__global__ __launch_bounds__(64 * kWaves) void k_seed_update(
    const double* __restrict__ X, int N, int A, const double* __restrict__ ctr, int first,
    double* __restrict__ w, double* __restrict__ R) {
  __shared__ double stage[kWaves][64 * kStride];
  const int lane = dmlp::lane_id(), wv = threadIdx.x >> 6;
  const int nruns = (N - 1) / 64 + 1;
  const int r = blockIdx.x * kWaves + wv;
  if (r >= nruns) return;   // (wave-uniform; no workgroup barrier below)
  const int row0 = r * 64;
  const int n = N - row0 < 64 ? N - row0 : 64;   // rows of this run
  double* t = stage[wv];
  // staging map: load k brings rows 4k .. 4k + 3, lane L row 4k + L / 16, column L % 16
  const int srow = lane >> 4, scol = lane & 15;
  const double* xs = X + (int64_t)row0 * A + (int64_t)srow * A + scol;
  double st[kChunk];
  auto load = [&](int64_t a0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < kChunk; ++k)
      st[k] = (4 * k + srow < n && a0 + scol < A) ? xs[(int64_t)(4 * k) * A + a0] : 0.0;
  };
  double s = 0.0;
  load(0);
  for (int64_t a0 = 0; a0 < A; a0 += kChunk) {
#pragma unroll
    for (int k = 0; k < kChunk; ++k) t[(4 * k + srow) * kStride + scol] = st[k];
    dmlp::wave_sync();
    if (A - a0 > kChunk) load(a0 + kChunk);
    const double* x = t + lane * kStride;
    const double* c = ctr + a0;
    if (A - a0 >= kChunk) {
#pragma unroll
      for (int a = 0; a < kChunk; ++a) {
        const double d = __dsub_rn(x[a], c[a]);
        s = __dadd_rn(s, __dmul_rn(d, d));
      }
    } else {
      for (int a = 0; a < (int)(A - a0); ++a) {
        const double d = __dsub_rn(x[a], c[a]);
        s = __dadd_rn(s, __dmul_rn(d, d));
      }
    }
    dmlp::wave_sync();   // the stage is read before the next chunk overwrites it
  }
  const bool live = lane < n;
  double wi = INFINITY;
  if (live && !first) wi = w[row0 + lane];
  wi = s < wi ? s : wi;   // (a NaN distance leaves w_i)
  if (live) w[row0 + lane] = wi;
  const double v = live && wi < INFINITY ? wi : 0.0;
  double before;
  const double Rr = lane_chain(0.0, v, before);
  if (lane == 0) R[r] = Rr;
}

// One wave walks items 0 .. n - 1 (val(i) >= +0.0) with the running sum s: the index of the first
// item with s + val > t, s then the sum BEFORE it; else -1, s the sum over all items and fb the
// last item with val > 0 (unchanged when there is none).
template <class Val>
__device__ __forceinline__ int wave_walk(int n, Val val, double& s, double t, int& fb) {
  const int lane = dmlp::lane_id();
  for (int g0 = 0; g0 < n; g0 += 64) {
    const bool in = lane < n - g0;
    const double v = in ? val(g0 + lane) : 0.0;
    double before = 0.0;
    const double end = lane_chain(s, v, before);
    const unsigned long long hit = __ballot(in && __dadd_rn(before, v) > t);
    const unsigned long long pos = __ballot(v > 0.0);
    if (hit) {
      const int L = __ffsll((long long)hit) - 1;
      s = __shfl(before, L);
      return g0 + L;
    }
    if (pos) fb = g0 + 63 - __clzll((long long)pos);
    s = end;
  }
  return -1;
}

// u == nullptr: step 0, the seed is i0
__global__ __launch_bounds__(kPickThreads) void k_seed_pick(
    const double* __restrict__ X, int N, int A, const double* __restrict__ w,
    const double* __restrict__ R, double* B, const double* __restrict__ u, int i0,
    int* __restrict__ seed_out, double* __restrict__ Cj) {
  __shared__ int pick;
  const int nruns = (N - 1) / 64 + 1, nblocks = (nruns - 1) / 64 + 1;
  if (u == nullptr) {
    if (threadIdx.x == 0) pick = i0;
  } else {
    for (int b = threadIdx.x; b < nblocks; b += kPickThreads) {
      const double* Rb = R + (int64_t)b * 64;
      const int n = nruns - b * 64 < 64 ? nruns - b * 64 : 64;
      double s = 0.0;
      for (int j0 = 0; j0 < n; j0 += kPickAhead) {
        double x[kPickAhead];
#pragma unroll
        for (int k = 0; k < kPickAhead; ++k) x[k] = j0 + k < n ? Rb[j0 + k] : 0.0;
#pragma unroll
        for (int k = 0; k < kPickAhead; ++k) s = __dadd_rn(s, x[k]);
      }
      B[b] = s;
    }
    __syncthreads();   // B, written above, is read by wave 0
    if (threadIdx.x < 64) {
      const double uj = *u;
      auto blocks = [&](int b) __attribute__((always_inline)) { return B[b]; };
      int fb = 0;
      double T = 0.0;
      wave_walk(nblocks, blocks, T, INFINITY, fb);
      int64_t row;
      if (!(T > 0.0 && T < INFINITY)) {
        const double p = __dmul_rn(uj, (double)N);
        row = p >= 0.0 ? (p < (double)N ? (int64_t)p : N - 1) : 0;   // (a NaN u: row 0)
      } else {
        const double t = __dmul_rn(uj, T);
        double s = 0.0;
        int b = wave_walk(nblocks, blocks, s, t, fb);
        b = b < 0 ? fb : b;
        fb = 0;
        const int nr = nruns - b * 64 < 64 ? nruns - b * 64 : 64;
        int rr = wave_walk(nr, [&](int i) __attribute__((always_inline)) {
          return R[(int64_t)b * 64 + i]; }, s, t, fb);
        rr = rr < 0 ? fb : rr;
        fb = 0;
        const int64_t i0r = ((int64_t)b * 64 + rr) * 64;
        const int ni = N - i0r < 64 ? (int)(N - i0r) : 64;
        int k = wave_walk(ni, [&](int i) __attribute__((always_inline)) {
          const double wi = w[i0r + i];
          return wi < INFINITY ? wi : 0.0; }, s, t, fb);
        k = k < 0 ? fb : k;
        row = i0r + k;
      }
      // whatever u holds, the row copied below exists
      if (threadIdx.x == 0) pick = (int)(row < 0 ? 0 : (row < N ? row : N - 1));
    }
  }
  __syncthreads();
  const int row = pick;
  if (threadIdx.x == 0) *seed_out = row;
  for (int a = threadIdx.x; a < A; a += kPickThreads) Cj[a] = X[(int64_t)row * A + a];
}

}  // namespace

extern "C" int64_t dmlp_kmeans_seed_bytes(int64_t N) {
  if (N < 0 || N > INT_MAX) return -1;
  const int64_t nruns = (N + 63) / 64;
  return (nruns + (nruns + 63) / 64) * (int64_t)sizeof(double);
}

extern "C" int dmlp_kmeans_seed(const double* X, int64_t N, int A, int K, int i0, const double* u,
                                int* seeds, double* C, double* w, void* ws, int64_t ws_bytes,
                                void* stream) {
  if (N <= 0 || K <= 0) return 0;
  if (N > INT_MAX || A < 1 || i0 < 0 || i0 >= N || !X || (K > 1 && !u) || !seeds || !C || !w ||
      !ws || ws_bytes < dmlp_kmeans_seed_bytes(N))
    return -1;
  hipStream_t st = (hipStream_t)stream;
  const int nruns = (int)((N + 63) / 64);
  double* R = (double*)ws;
  double* B = R + nruns;
  const dim3 ugrid((unsigned)((nruns + kWaves - 1) / kWaves));
  for (int j = 0; j < K; ++j) {
    if (j > 0) {
      hipLaunchKernelGGL(k_seed_update, ugrid, dim3(64 * kWaves), 0, st, X, (int)N, A,
                         (const double*)(C + (int64_t)(j - 1) * A), j == 1 ? 1 : 0, w, R);
      DMLP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_seed_pick, dim3(1), dim3(kPickThreads), 0, st, X, (int)N, A,
                       (const double*)w, (const double*)R, B, j > 0 ? u + (j - 1) : nullptr, i0,
                       seeds + j, C + (int64_t)j * A);
    DMLP_LAUNCH_CHECK();
  }
  // w belongs to all K seeds
  hipLaunchKernelGGL(k_seed_update, ugrid, dim3(64 * kWaves), 0, st, X, (int)N, A,
                     (const double*)(C + (int64_t)(K - 1) * A), K == 1 ? 1 : 0, w, R);
  DMLP_LAUNCH_CHECK();
  return 0;
}
