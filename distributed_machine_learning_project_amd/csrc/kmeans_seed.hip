// kmeans_seed.hip — D^2 (k-means++) seeding on the device (dmlp.h: k-means seeding, and its greedy
// variant with local trials), bit-identical to dmlp_cpu_kmeans_seed / dmlp_cpu_kmeans_seed_trials:
// no FMA, no floating-point atomics, every sum in the contract's fixed order (rows in runs of 64,
// runs in blocks of 64, the blocks left to right).  The random numbers u come from the caller, so
// a seeding is 2K launches (2K + 2 with local trials) on one stream without a host sync.
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
// Local trials (dmlp_kmeans_seed_trials): L candidates per step, the one with the least potential
// is kept.  The workspace holds m [L][N] (trial l's minima), R [L][nruns], B [L][nblocks], the
// candidate rows [L][A], then the words l* and the L candidate row ids.
//   k_seed_trial<LB>   once per step, the hot kernel: k_seed_update's staged pass (staged_dists,
//     shared) with LB distance chains per lane, one per candidate, so X is read once for all of
//     them and the chains are independent of each other.  The candidate rows are wave-uniform
//     reads of the workspace's slab.  LB >= L is a compile-time bound (the chains live in
//     registers); a chain past the live ones repeats the last candidate and is stored nowhere.
//     The commit of the step before is folded in: the lane's w_i is m[l*][i], l* the device word
//     the pick wrote (step 0: +inf), and the lane writes m[l][i] for every live l in place — a
//     row is touched by its own lane only.  Then the L run sums by L interleaved lane chains.
//   k_seed_pick_trials one workgroup per step, after the step's trials.  (1) its threads take the
//     (l, b) pairs: B_l[b], 64 run sums in order; (2) thread l adds trial l's block sums left to
//     right: P_l; thread 0 takes the smallest l with the least P_l, publishes l* and seeds[j],
//     and the workgroup copies the winner's row out of the slab into C[j]; (3) with trial l*'s B,
//     R and m the four waves walk a candidate each (pick_row, k_seed_pick's walk) with u[j][l];
//     (4) the workgroup writes the candidates' ids and rows into the slab.  Step 0's pick only
//     writes candidate i0; the pick after the last trial stops after (2).
//   k_seed_commit      once, at the end: w = m[l*].  It is a grid of its own, not the tail of the
//     last pick, which is one workgroup: 8 N bytes through one compute unit would cost more than
//     the launch.
//
// A lane past the end of a short run (or a thread past the last run of a block) adds 0.0 to the
// chain: every sum here is >= +0.0 (v_i >= +0.0, never NaN), and s + 0.0 == s bit for bit for such
// s, so the short run's sum is the contract's.
#include "dmlp.h"
#include "dmlp_device.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int kWaves = 4;             // waves (runs) per workgroup of k_seed_update / k_seed_trial
constexpr int kChunk = 16;            // attributes per LDS stage
constexpr int kStride = kChunk + 1;   // doubles per staged row: odd
constexpr int kPickThreads = 256;
constexpr int kPickAhead = 16;        // run sums in flight ahead of a block's add chain
constexpr int kMaxTrials = 16;
constexpr int kCommitThreads = 256;

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

// LB of those chains from 0.0, interleaved: s[l] = ((v[l]_0 + v[l]_1) + ...) + v[l]_63
template <int LB>
__device__ __forceinline__ void lane_chains(double (&s)[LB], const double (&v)[LB]) {
#pragma unroll
  for (int l = 0; l < LB; ++l) s[l] = 0.0;
#pragma unroll 4
  for (int L = 0; L < 64; ++L) {
#pragma unroll
    for (int l = 0; l < LB; ++l) s[l] = __dadd_rn(s[l], lane_bcast(v[l], L));
  }
}

// The staged pass of a wave over its run (rows row0 .. row0 + n - 1, the lane is the row) against
// LB centre rows, centre l at ctr + min(l, live - 1) * A: s[l] = d(x_lane, centre l), the
// attributes in order.  t: the wave's own 64 * kStride doubles of LDS.
template <int LB>
__device__ __forceinline__ void staged_dists(const double* __restrict__ X, int A, int row0, int n,
                                             double* t, const double* __restrict__ ctr, int live,
                                             double (&s)[LB]) {
  const int lane = dmlp::lane_id();
  // staging map: load k brings rows 4k .. 4k + 3, lane L row 4k + L / 16, column L % 16
  const int srow = lane >> 4, scol = lane & 15;
  const double* xs = X + (int64_t)row0 * A + (int64_t)srow * A + scol;
  const double* cl[LB];
#pragma unroll
  for (int l = 0; l < LB; ++l) {
    cl[l] = ctr + (int64_t)(l < live ? l : live - 1) * A;
    s[l] = 0.0;
  }
  double st[kChunk];
  auto load = [&](int64_t a0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < kChunk; ++k)
      st[k] = (4 * k + srow < n && a0 + scol < A) ? xs[(int64_t)(4 * k) * A + a0] : 0.0;
  };
  load(0);
  for (int64_t a0 = 0; a0 < A; a0 += kChunk) {
#pragma unroll
    for (int k = 0; k < kChunk; ++k) t[(4 * k + srow) * kStride + scol] = st[k];
    dmlp::wave_sync();
    if (A - a0 > kChunk) load(a0 + kChunk);
    const double* x = t + lane * kStride;
    if (A - a0 >= kChunk) {
#pragma unroll
      for (int a = 0; a < kChunk; ++a) {
        const double xa = x[a];
#pragma unroll
        for (int l = 0; l < LB; ++l) {
          const double d = __dsub_rn(xa, cl[l][a0 + a]);
          s[l] = __dadd_rn(s[l], __dmul_rn(d, d));
        }
      }
    } else {
      for (int a = 0; a < (int)(A - a0); ++a) {
        const double xa = x[a];
#pragma unroll
        for (int l = 0; l < LB; ++l) {
          const double d = __dsub_rn(xa, cl[l][a0 + a]);
          s[l] = __dadd_rn(s[l], __dmul_rn(d, d));
        }
      }
    }
    dmlp::wave_sync();   // the stage is read before the next chunk overwrites it
  }
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
  double s[1];
  staged_dists<1>(X, A, row0, n, stage[wv], ctr, 1, s);
  const bool live = lane < n;
  double wi = INFINITY;
  if (live && !first) wi = w[row0 + lane];
  wi = s[0] < wi ? s[0] : wi;   // (a NaN distance leaves w_i)
  if (live) w[row0 + lane] = wi;
  const double v = live && wi < INFINITY ? wi : 0.0;
  double before;
  const double Rr = lane_chain(0.0, v, before);
  if (lane == 0) R[r] = Rr;
}

// live (<= LB) trials of the slab's candidates against w = m[*lstar] (first: +inf)
template <int LB>
__global__ __launch_bounds__(64 * kWaves) void k_seed_trial(
    const double* __restrict__ X, int N, int A, const double* __restrict__ cand, int live,
    int first, const int* __restrict__ lstar, double* m, double* __restrict__ R) {
  __shared__ double stage[kWaves][64 * kStride];
  const int lane = dmlp::lane_id(), wv = threadIdx.x >> 6;
  const int nruns = (N - 1) / 64 + 1;
  const int r = blockIdx.x * kWaves + wv;
  if (r >= nruns) return;   // (wave-uniform; no workgroup barrier below)
  const int row0 = r * 64;
  const int n = N - row0 < 64 ? N - row0 : 64;
  double s[LB];
  staged_dists<LB>(X, A, row0, n, stage[wv], cand, live, s);
  const bool in = lane < n;
  double wi = INFINITY;
  if (in && !first) wi = m[(int64_t)*lstar * N + row0 + lane];
  double v[LB];
#pragma unroll
  for (int l = 0; l < LB; ++l) {
    const double ml = s[l] < wi ? s[l] : wi;   // (a NaN distance leaves w_i)
    if (in && l < live) m[(int64_t)l * N + row0 + lane] = ml;
    v[l] = in && ml < INFINITY ? ml : 0.0;
  }
  lane_chains<LB>(s, v);
#pragma unroll
  for (int l = 0; l < LB; ++l)
    if (lane == 0 && l < live) R[(int64_t)l * nruns + r] = s[l];
}

// p[0] + p[1] + ... + p[n - 1] left to right from 0.0, by one thread
__device__ __forceinline__ double sum_lr(const double* p, int n) {
  double s = 0.0;
  for (int j0 = 0; j0 < n; j0 += kPickAhead) {
    double x[kPickAhead];
#pragma unroll
    for (int k = 0; k < kPickAhead; ++k) x[k] = j0 + k < n ? p[j0 + k] : 0.0;
#pragma unroll
    for (int k = 0; k < kPickAhead; ++k) s = __dadd_rn(s, x[k]);
  }
  return s;
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

// The contract's pick (step 3) by one wave: the row for the draw uj, given the total T of the
// block sums B over the run sums R over the rows' w; clamped into [0, N) whatever uj holds.
__device__ __forceinline__ int pick_row(int N, const double* B, const double* R, const double* w,
                                        double T, double uj) {
  const int nruns = (N - 1) / 64 + 1, nblocks = (nruns - 1) / 64 + 1;
  int64_t row;
  if (!(T > 0.0 && T < INFINITY)) {
    const double p = __dmul_rn(uj, (double)N);
    row = p >= 0.0 ? (p < (double)N ? (int64_t)p : N - 1) : 0;   // (a NaN u: row 0)
  } else {
    const double t = __dmul_rn(uj, T);
    double s = 0.0;
    int fb = 0;
    int b = wave_walk(nblocks, [&](int i) __attribute__((always_inline)) { return B[i]; }, s, t,
                      fb);
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
  return (int)(row < 0 ? 0 : (row < N ? row : N - 1));
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
    for (int b = threadIdx.x; b < nblocks; b += kPickThreads)
      B[b] = sum_lr(R + (int64_t)b * 64, nruns - b * 64 < 64 ? nruns - b * 64 : 64);
    __syncthreads();   // B, written above, is read by wave 0
    if (threadIdx.x < 64) {
      int fb = 0;
      double T = 0.0;
      wave_walk(nblocks, [&](int b) __attribute__((always_inline)) { return B[b]; }, T, INFINITY,
                fb);
      // whatever u holds, the row copied below exists
      const int row = pick_row(N, B, R, w, T, *u);
      if (threadIdx.x == 0) pick = row;
    }
  }
  __syncthreads();
  const int row = pick;
  if (threadIdx.x == 0) *seed_out = row;
  for (int a = threadIdx.x; a < A; a += kPickThreads) Cj[a] = X[(int64_t)row * A + a];
}

// nprev: the live trials of the step before (0: step 0, candidate i0 and nothing else);
// u: the L draws of this step (nullptr: after the last trial, no new candidates).
// st: the word l*, then the candidate row ids.
__global__ __launch_bounds__(kPickThreads) void k_seed_pick_trials(
    const double* __restrict__ X, int N, int A, int L, int nprev, const double* __restrict__ u,
    int i0, const double* m, const double* R, double* B, double* cand, int* st, int* seed_out,
    double* Cj) {
  __shared__ double P[kMaxTrials];
  __shared__ int rows[kMaxTrials];
  __shared__ int best;
  const int nruns = (N - 1) / 64 + 1, nblocks = (nruns - 1) / 64 + 1;
  int ncand = 1;
  if (nprev == 0) {
    if (threadIdx.x == 0) rows[0] = i0;
  } else {
    for (int i = threadIdx.x; i < nprev * nblocks; i += kPickThreads) {
      const int l = i / nblocks, b = i - l * nblocks;
      B[i] = sum_lr(R + (int64_t)l * nruns + (int64_t)b * 64,
                    nruns - b * 64 < 64 ? nruns - b * 64 : 64);
    }
    __syncthreads();   // B, written above, is read by other threads
    if (threadIdx.x < nprev) P[threadIdx.x] = sum_lr(B + (int64_t)threadIdx.x * nblocks, nblocks);
    __syncthreads();
    if (threadIdx.x == 0) {
      int bl = 0;
      for (int l = 1; l < nprev; ++l) bl = P[l] < P[bl] ? l : bl;   // (P is never NaN)
      best = bl;
      st[0] = bl;
      *seed_out = st[1 + bl];
    }
    __syncthreads();
    const int bl = best;
    for (int a = threadIdx.x; a < A; a += kPickThreads) Cj[a] = cand[(int64_t)bl * A + a];
    if (u == nullptr) return;
    for (int l = threadIdx.x >> 6; l < L; l += kPickThreads / 64) {   // (wave-uniform)
      const int row = pick_row(N, B + (int64_t)bl * nblocks, R + (int64_t)bl * nruns,
                               m + (int64_t)bl * N, P[bl], u[l]);
      if (dmlp::lane_id() == 0) rows[l] = row;
    }
    ncand = L;
  }
  __syncthreads();   // the slab's winner is copied out, the new rows are known
  if (threadIdx.x < ncand) st[1 + threadIdx.x] = rows[threadIdx.x];
  for (int i = threadIdx.x; i < ncand * A; i += kPickThreads) {
    const int l = i / A, a = i - l * A;
    cand[i] = X[(int64_t)rows[l] * A + a];
  }
}

__global__ __launch_bounds__(kCommitThreads) void k_seed_commit(
    const double* __restrict__ m, int N, const int* __restrict__ lstar, double* __restrict__ w) {
  const int i = blockIdx.x * kCommitThreads + threadIdx.x;
  if (i < N) w[i] = m[(int64_t)*lstar * N + i];
}

// the workspace of the trials, in doubles: m, R, B, the slab, then the state words
struct TrialWs {
  int64_t m, R, B, cand, st, bytes;
};

TrialWs trial_ws(int64_t N, int A, int L) {
  const int64_t nruns = (N + 63) / 64, nblocks = (nruns + 63) / 64;
  TrialWs o;
  o.m = 0;
  o.R = o.m + L * N;
  o.B = o.R + L * nruns;
  o.cand = o.B + L * nblocks;
  o.st = o.cand + (int64_t)L * A;
  o.bytes = (o.st + (1 + L + 1) / 2) * (int64_t)sizeof(double);
  return o;
}

template <int LB>
void launch_trial(dim3 grid, hipStream_t st, const double* X, int N, int A, const double* cand,
                  int live, int first, const int* lstar, double* m, double* R) {
  hipLaunchKernelGGL(k_seed_trial<LB>, grid, dim3(64 * kWaves), 0, st, X, N, A, cand, live, first,
                     lstar, m, R);
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

extern "C" int64_t dmlp_kmeans_seed_trials_bytes(int64_t N, int A, int L) {
  if (N < 0 || N > INT_MAX || A < 1 || L < 1 || L > kMaxTrials) return -1;
  return trial_ws(N, A, L).bytes;
}

extern "C" int dmlp_kmeans_seed_trials(const double* X, int64_t N, int A, int K, int L, int i0,
                                       const double* u, int* seeds, double* C, double* w, void* ws,
                                       int64_t ws_bytes, void* stream) {
  if (N <= 0 || K <= 0) return 0;
  if (N > INT_MAX || A < 1 || L < 1 || L > kMaxTrials || i0 < 0 || i0 >= N || !X ||
      (K > 1 && !u) || !seeds || !C || !w || !ws || ws_bytes < trial_ws(N, A, L).bytes)
    return -1;
  hipStream_t st = (hipStream_t)stream;
  const TrialWs o = trial_ws(N, A, L);
  double* base = (double*)ws;
  double *m = base + o.m, *R = base + o.R, *B = base + o.B, *cand = base + o.cand;
  int* state = (int*)(base + o.st);
  const int nruns = (int)((N + 63) / 64);
  const dim3 tgrid((unsigned)((nruns + kWaves - 1) / kWaves));
  // steps 0 .. K - 1: the candidates, then their trials; j == K: the last winner only
  for (int j = 0; j <= K; ++j) {
    const int nprev = j == 0 ? 0 : (j == 1 ? 1 : L);
    hipLaunchKernelGGL(k_seed_pick_trials, dim3(1), dim3(kPickThreads), 0, st, X, (int)N, A, L,
                       nprev, j > 0 && j < K ? u + (int64_t)(j - 1) * L : nullptr, i0,
                       (const double*)m, (const double*)R, B, cand, state,
                       seeds + (j > 0 ? j - 1 : 0), C + (int64_t)(j > 0 ? j - 1 : 0) * A);
    DMLP_LAUNCH_CHECK();
    if (j == K) break;
    const int live = j == 0 ? 1 : L, first = j == 0 ? 1 : 0;
#define DMLP_TRIAL(LB)                                                                         \
  launch_trial<LB>(tgrid, st, X, (int)N, A, (const double*)cand, live, first, (const int*)state, \
                   m, R)
    // the smallest compiled bound that holds the live trials
    if (live <= 1) DMLP_TRIAL(1);
    else if (live <= 2) DMLP_TRIAL(2);
    else if (live <= 3) DMLP_TRIAL(3);
    else if (live <= 4) DMLP_TRIAL(4);
    else if (live <= 5) DMLP_TRIAL(5);
    else if (live <= 6) DMLP_TRIAL(6);
    else if (live <= 7) DMLP_TRIAL(7);
    else if (live <= 8) DMLP_TRIAL(8);
    else if (live <= 10) DMLP_TRIAL(10);
    else if (live <= 12) DMLP_TRIAL(12);
    else DMLP_TRIAL(16);
#undef DMLP_TRIAL
    DMLP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_seed_commit, dim3((unsigned)((N + kCommitThreads - 1) / kCommitThreads)),
                     dim3(kCommitThreads), 0, st, (const double*)m, (int)N, (const int*)state, w);
  DMLP_LAUNCH_CHECK();
  return 0;
}
