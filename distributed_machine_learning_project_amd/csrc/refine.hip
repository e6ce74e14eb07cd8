// refine.hip — exact re-ranking of the screen's survivors, one query per wave, and the host
// entry points of every refine (the two-queries-per-wave kernel itself: refine_pair.hip).
//
//  * k_refine   : exact fp64 distances (reference order, no FMA: engine.cpp:12-18) of the
//                 screen's survivors and an exact top-k under (dist asc, id desc)
//                 (SURVEY.md §2.5 K2/K3/K6).  One wave per query; a P-slot running top-k in
//                 LDS absorbs 64 candidates per step and is re-sorted (register bitonic) only
//                 when full.  Vote + FNV checksum are fused when labels are given (K5/K7).
//  * k_finalize : that vote (max count, tie -> larger label; engine.cpp:319-332) + FNV-1a
//                 checksum (common.cpp:59-70) alone, of lists already sorted.  It shares
//                 finalize_wave with k_refine's tail and is kept in this file for it: compiled in
//                 a file where it is finalize_wave's only caller its code comes out different
//                 (22 VGPRs for 18, another block layout: profiles/refine_split.md).
//  * dmlp_refine (id lists) and dmlp_refine_groups* (the single-term screen's group entries),
//    which share refine_groups_impl; dmlp_refine_pair_path tells which kernel serves a list.
#include "dmlp.h"
#include "dmlp_device.h"
#include "refine_common.h"
#include <float.h>

namespace {

constexpr int kHistCap = 512;  // per-wave label histogram (labels in [lo, lo+512))

// the same over a lossless int32 row, each value divided back exactly as k_rows_from_i32 does
__device__ __forceinline__ double exact_dist_row_i32(const double* __restrict__ q,
                                                     const int* __restrict__ x, int A) {
  double s = 0.0;
  for (int a = 0; a < A; ++a) {
    const double d = __dsub_rn(q[a], (double)x[a] / 1.0e6);
    s = __dadd_rn(s, __dmul_rn(d, d));
  }
  return s;
}

__device__ __forceinline__ double exact_dist_row(const double* __restrict__ q,
                                                 const double* __restrict__ x, int A) {
  double s = 0.0;
  if ((A & 1) == 0) {
    const double2* x2 = (const double2*)x;
    for (int a = 0; a < (A >> 1); ++a) {
      const double2 v = x2[a];
      const double d0 = __dsub_rn(q[2 * a], v.x);
      s = __dadd_rn(s, __dmul_rn(d0, d0));
      const double d1 = __dsub_rn(q[2 * a + 1], v.y);
      s = __dadd_rn(s, __dmul_rn(d1, d1));
    }
  } else {
    for (int a = 0; a < A; ++a) {
      const double d = __dsub_rn(q[a], x[a]);
      s = __dadd_rn(s, __dmul_rn(d, d));
    }
  }
  return s;
}

// Running top-k of one wave, P = E*64 slots in LDS: [0,k) current best (sorted), new
// candidates appended at k+fill; re-sorted when fewer than 64 free slots remain.
template <int E>
struct RunTopK {
  static constexpr int P = E * 64;
  double* d;
  int* id;
  int k;
  int fill;
  __device__ void init(double* d_, int* id_, int k_) {
    d = d_; id = id_; k = k_; fill = 0;
    for (int i = dmlp::lane_id(); i < P; i += 64) { d[i] = INFINITY; id[i] = -1; }
    dmlp::wave_sync();
  }
  __device__ void flush() {
    if (fill == 0) return;
    double rd[E]; int ri[E];
    const int lane = dmlp::lane_id();
    dmlp::wave_sync();
#pragma unroll
    for (int r = 0; r < E; ++r) { rd[r] = d[r * 64 + lane]; ri[r] = id[r * 64 + lane]; }
    dmlp::wave_sort_keys<E>(rd, ri);
    dmlp::wave_sync();
#pragma unroll
    for (int r = 0; r < E; ++r) {
      const int i = r * 64 + lane;
      d[i] = i < k ? rd[r] : INFINITY;
      id[i] = i < k ? ri[r] : -1;
    }
    dmlp::wave_sync();
    fill = 0;
  }
  __device__ void push(bool valid, double dv, int iv) {
    const unsigned long long m = __ballot(valid);
    if (valid) {
      const int pos = k + fill + __popcll(m & dmlp::lanemask_lt());
      d[pos] = dv;
      id[pos] = iv;
    }
    fill += __popcll(m);
    if (k + fill + 64 > P) flush();
  }
};

__device__ __forceinline__ void finalize_wave(const int* ids, int k, const int* __restrict__ labels,
                                              int label_lo, int label_hi, int* hist,
                                              int* out_label, uint64_t* out_cs,
                                              int hist_cap = kHistCap) {
  const int lane = dmlp::lane_id();
  // labels of ids < 0 (padding) are never read
  const int label = k > 0 ? dmlp::wave_vote(ids, k, labels, label_lo, label_hi, hist, hist_cap) : -1;
  if (lane == 0) {
    *out_label = label;
    *out_cs = dmlp::fnv_checksum(label, ids, k);
  }
}

// Group-mode inputs (single-term screen, screen_x1.hip): candidates are 4-row group entries
// (ordered 16-bit group-max key << 16 | slice-relative group index) and cand_h holds each
// slice's final threshold and the query's screen error bound eps.  The k-th largest key over all slices gives h = a_k' - 2 eps (a lower
// bound on a_k - eps, exactly the screen's own rule, but global); a member survives iff its
// single-term score  s = -|x'|^2/2 + <hi(q'), hi(x')>  (recomputed from the screen's image: bf16
// for hl = 2, fp16 for hl = 1;
// any summation order obeys the same error bound) is >= h.  Only survivors get exact distances.
struct GroupIn {
  const float* cand_h;    // [nq * S][2]: slice threshold, query eps
  const u32x4* xfrag;     // tile image (hi first; hl = 2: prep.hip's hi/lo, 1: hi only)
  const float* xinit;     // -|x'|^2/2 per point
  const bf16x8* qhi;      // [Q][KT*4] query hi fragments
  int KT;
  int hl;
  int n_points;
  int tiles_per_slice;    // the screen's slicing: group base = (s * tps * 64) + 4 * index
  int collect;            // lists of the COLLECT pass (large k): the threshold is always taken
                          // over the lists (cand_h holds the fixed seed, not a final threshold)
  int rescore = 1;        // 0 (screen_f64.hip's fp64 keys): every member of a group at or above
                          // the threshold goes to the exact re-rank (no image to rescore from)
  int grows = 4;          // rows per group entry: 4 (consecutive) or 8 (the SUB = 16 screen's pair
                          // epilogue: rows 4 kg + i of steps 2p and 2p + 1, entry = 4 p + kg)
  const int* xi32 = nullptr;  // the dataset's lossless int32 rows (X unused), or null
};

// GROUPS = KT of the single-term screen (1, 2, 4 or 8) for group-mode input, 0 otherwise.  The group
// variant sizes its LDS for k <= 32 (the screen's limit) and labels in [lo, lo + 256) (wider
// label ranges take wave_vote's counting fallback), so more waves stay resident to hide the
// gathers that dominate this kernel.
// E = 8 with GROUPS: the large-k group variant (k <= 256 over <= 512 filtered members): its
// top-k is one wave-wide bitonic sort of the members' exact keys, and labels are gathered at the
// vote (no carry scratch).
template <int E, int GROUPS, bool F16 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((GROUPS && E >= 8) ? 2 : GROUPS == 1 ? 8 : GROUPS ? 4 : 1))) void k_refine(
    const int* __restrict__ cand_ids, const int* __restrict__ cand_cnt, int S, int cap,
    const double* __restrict__ X, int A, const double* __restrict__ Qx,
    const int* __restrict__ qidx, const int* __restrict__ qk, int nq, double* __restrict__ out_d,
    int* __restrict__ out_i, int kstride, const int* __restrict__ labels, int label_lo,
    int label_hi, int* __restrict__ out_label, uint64_t* __restrict__ out_cs,
    int* __restrict__ status, int* __restrict__ ovf_count, const GroupIn gin) {
  constexpr int P = E * 64;
  constexpr int SMAX = 256;
  constexpr bool GBIG = GROUPS && E >= 8;
  constexpr int KMAX = GBIG ? 256 : GROUPS ? 64 : 128;
  constexpr int HCAP = GROUPS ? 256 : kHistCap;  // >= 256: the key histogram of the global threshold
  __shared__ double s_d[4][P];
  __shared__ int s_i[4][P];
  __shared__ double s_rd[4][KMAX];
  __shared__ int s_ri[4][KMAX];
  __shared__ int s_pre[4][SMAX + 1];
  __shared__ __attribute__((aligned(16))) int s_hist[4][HCAP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x * 4 + wave;
  if (p >= nq) return;
  // qidx == nullptr: every query in order (no dependent index load at the head of the chain)
  const int q = qidx ? __builtin_amdgcn_readfirstlane(qidx[p]) : p;
  const int k = __builtin_amdgcn_readfirstlane(qk[q]);
  const int* cnt = cand_cnt + (int64_t)p * S;
  // group mode: everything that depends only on (p, q) is requested here, in one batch, instead
  // of one dependent latency after another (this kernel is bound by its chain of gathers)
  constexpr int KTG = GROUPS ? GROUPS : 1;
  // A > 64 (KT = 4, 8): hi(q') is read from LDS at each use (staged below) — 64 / 128 registers
  // held through the member loop would spill
  constexpr bool QLDS = GROUPS >= 4;
  u32x4 qraw[QLDS ? 1 : KTG * 4];
  float g_eps = 0.0f, g_h1 = 0.0f;
  unsigned ebuf = 0;  // S == 1: entry `lane` of the query's single slice
  if (GROUPS) {
    if (KTG == 1 && gin.rescore) {  // (KT = 2: 32 registers held this long would spill; loaded at first use)
#pragma unroll
      for (int f = 0; f < KTG * 4; ++f)
        qraw[f] = __builtin_bit_cast(u32x4, gin.qhi[(int64_t)q * KTG * 4 + f]);
    }
    g_eps = gin.cand_h[2 * (int64_t)p * S + 1];
    g_h1 = gin.cand_h[2 * (int64_t)p * S];  // slice 0's (COLLECT: every slice holds the seed)
    if (S == 1 && lane < cap) ebuf = (unsigned)cand_ids[(int64_t)p * cap + lane];
  }
  // prefix of candidate counts over slices (S <= SMAX); group mode: the largest eps over the
  // slices — a screen launched per data chunk (pipeline.hip's large-N pipeline) bounds each
  // slice's error with the image's max norm seen so far, and the global threshold must hold for
  // every slice's members (a_k' - 2 max eps <= a_k - eps of any member)
  int* pre = s_pre[wave];
  bool ovf = false;
  if (lane == 0) {
    int acc = 0;
    pre[0] = 0;
    for (int s = 0; s < S; ++s) {
      const int n = cnt[s];
      if (n < 0) ovf = true;
      acc += n < 0 ? 0 : n;
      pre[s + 1] = acc;
      if (GROUPS && s > 0) g_eps = fmaxf(g_eps, gin.cand_h[2 * ((int64_t)p * S + s) + 1]);
    }
  }
  ovf = __shfl(ovf ? 1 : 0, 0) != 0;
  if (GROUPS) g_eps = __shfl(g_eps, 0);
  // the (+inf, -1) padding of slots [k, kstride) is written here, so callers need no fill pass
  // (slots [0, k) of a query handed back below are written by its escalation / exact path)
  for (int i = k + lane; i < kstride; i += 64) {
    out_d[(int64_t)q * kstride + i] = INFINITY;
    out_i[(int64_t)q * kstride + i] = -1;
  }
  if (ovf) {
    if (lane == 0) {
      status[q] = 1;
      if (ovf_count) atomicAdd(ovf_count, 1);  // running total: the host reads 4 bytes
    }
    return;
  }
  if (lane == 0) status[q] = 0;
  dmlp::wave_sync();
  int M = pre[S];
  const double* qv = Qx + (int64_t)q * A;
  auto slice_of = [&](int j) {
    // slice containing flat index j: largest s with pre[s] <= j
    int lo = 0, hi = S;  // pre[lo] <= j < pre[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (pre[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
  };
  auto cand = [&](int j, double& dv, int& id) {
    if (GROUPS) {
      id = s_i[wave][j];  // filtered members, staged below
    } else {
      const int lo = slice_of(j);
      id = cand_ids[((int64_t)p * S + lo) * cap + (j - pre[lo])];
    }
    dv = gin.xi32 ? exact_dist_row_i32(qv, gin.xi32 + (int64_t)id * A, A)
                  : exact_dist_row(qv, X + (int64_t)id * A, A);
  };
  if (GROUPS) {
    // ---- global threshold: k-th largest group key over all slices (two 8-bit histogram passes)
    auto entry = [&](int j) {
      const int lo = slice_of(j);
      return (unsigned)cand_ids[((int64_t)p * S + lo) * cap + (j - pre[lo])];
    };
    int* hist = s_hist[wave];
    const float eps = g_eps;
    // one slice: its final threshold is already global; COLLECT lists: the fixed seed (a valid
    // bound every slice shares), raised below to the k-th largest key over the lists
    float hq = S == 1 || gin.collect ? g_h1 : -INFINITY;
    if ((S > 1 || gin.collect) && M >= k && k >= 1) {
      int above = 0;
      int b1 = -1, b2 = -1;
#pragma unroll 1
      for (int pass = 0; pass < 2; ++pass) {
        for (int i = lane; i < 256; i += 64) hist[i] = 0;
        dmlp::wave_sync();
        for (int j = lane; j < M; j += 64) {
          const unsigned e = entry(j);
          if (pass == 0) atomicAdd(&hist[e >> 24], 1);
          else if ((int)(e >> 24) == b1) atomicAdd(&hist[(e >> 16) & 255], 1);
        }
        dmlp::wave_sync();
        const int b = dmlp::wave_kth_bin(hist, k - above, above);
        dmlp::wave_sync();
        if (pass == 0) b1 = b; else b2 = b;
      }
      const unsigned T = ((unsigned)b1 << 24) | ((unsigned)b2 << 16);
      const unsigned tb = T ^ ((T >> 31) ? 0x80000000u : 0xffffffffu);  // ordered -> fp32 bits
      hq = fmaxf(hq, __uint_as_float(tb) - 2.0f * eps);
    }
    const unsigned tq = __float_as_uint(hq);
    const unsigned kh = (tq ^ ((unsigned)((int)tq >> 31) | 0x80000000u)) & 0xffff0000u;
    // ---- expand surviving groups; keep members whose single-term score reaches hq
    constexpr int KT = GROUPS ? GROUPS : 1;  // (dead code for GROUPS == 0)
    // hi(q') stays packed (two bf16 per dword, 16 VGPRs per KT): unpacked at each use — a
    // 32-float copy would push this 64-register kernel into scratch spills
    u32x4* const qs = (u32x4*)s_hist[wave];  // (the histogram is dead once hq is known)
    if constexpr (QLDS) {
      static_assert(KT * 4 * 16 <= HCAP * 4, "query fragments must fit the histogram scratch");
      for (int f = lane; f < KT * 4 && gin.rescore; f += 64)
        qs[f] = __builtin_bit_cast(u32x4, gin.qhi[(int64_t)q * KT * 4 + f]);
      dmlp::wave_sync();
    } else if (KT != 1 && gin.rescore) {
#pragma unroll
      for (int f = 0; f < KT * 4; ++f)
        qraw[f] = __builtin_bit_cast(u32x4, gin.qhi[(int64_t)q * KT * 4 + f]);
    }
    // one member per lane (4 lanes per group: their fragments are adjacent 16-byte chunks).
    // Entries are fetched 64 groups at a time, one per lane, and dealt to the member lanes by
    // a shuffle: each 64-member step then waits on one gather (the fragments), not two.
    int nm = 0;
    const int GR = gin.grows, GS = GR == 8 ? 3 : 2;  // members per group entry, log2
    for (int j0 = 0; j0 < GR * M; j0 += 64) {
      const int jm = j0 + lane;
      const int g = jm >> GS;
      // S == 1: block 0 was fetched up front
      if ((j0 & (64 * GR - 1)) == 0 && (S > 1 || j0 > 0)) {
        const int gg = (j0 >> GS) + lane;
        ebuf = 0;
        if (gg < M) {
          const int lo = slice_of(gg);
          ebuf = (unsigned)cand_ids[((int64_t)p * S + lo) * cap + (gg - pre[lo])];
        }
      }
      const unsigned e = (unsigned)__shfl((int)ebuf, g & 63);
      int id = 0;
      bool keep = false;
      if (g < M) {
        const int lo = slice_of(g);
        id = lo * gin.tiles_per_slice * 64 + dmlp::group_row(e & 0xffffu, jm & (GR - 1), GR);
        if (e >= kh && id < gin.n_points && !gin.rescore) {
          keep = true;
        } else if (e >= kh && id < gin.n_points) {
          const int64_t t = id >> 6;
          const int pl = id & 63;
          const u32x4* fr = gin.xfrag + t * (int64_t)(4 * KT * gin.hl * 64) + (pl & 15);
          float sc = gin.xinit[id];
          // F16: the host's fp16 image + fp16 query fragments (hl = 1); else bf16 (a template
          // parameter: both decodes in one body pushed this 64-VGPR kernel into scratch spills)
#pragma unroll
          for (int kt = 0; kt < KT; ++kt) {
            const u32x4* fk = fr + (int64_t)(((pl >> 4) * KT + kt) * gin.hl) * 64;
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) {
              const u32x4 w = fk[16 * kq];
              const u32x4 qv = QLDS ? qs[kt * 4 + kq] : qraw[QLDS ? 0 : kt * 4 + kq];
#pragma unroll
              for (int q2 = 0; q2 < 4; ++q2) {
                const unsigned qw = qv[q2];
                if constexpr (F16) {  // products exact in fp32 either way: any order obeys the bound
                  sc += (float)__builtin_bit_cast(_Float16, (unsigned short)(qw & 0xffffu)) *
                        (float)__builtin_bit_cast(_Float16, (unsigned short)(w[q2] & 0xffffu));
                  sc += (float)__builtin_bit_cast(_Float16, (unsigned short)(qw >> 16)) *
                        (float)__builtin_bit_cast(_Float16, (unsigned short)(w[q2] >> 16));
                } else {
                  sc += __uint_as_float(qw << 16) * __uint_as_float(w[q2] << 16);
                  sc += __uint_as_float(qw & 0xffff0000u) * __uint_as_float(w[q2] & 0xffff0000u);
                }
              }
            }
          }
          keep = sc >= hq;
        }
      }
      const unsigned long long km = __ballot(keep);
      const int pos = nm + __popcll(km & dmlp::lanemask_lt());
      if (keep && pos < P) s_i[wave][pos] = id;
      nm += __popcll(km);
    }
    if (nm > P) {
      // pathological ties: hand the query back (x1 overflow -> 3-term screen escalation)
      if (lane == 0) {
        status[q] = 1;
        if (ovf_count) atomicAdd(ovf_count, 1);
      }
      return;
    }
    M = nm;
    dmlp::wave_sync();
  }
  const double* res_d;
  const int* res_i;
  // group mode: each candidate's label is gathered beside its row and travels with it (in the
  // slice-prefix scratch, dead after the member filter), so the vote reads LDS, not a final
  // dependent gather.  cl: candidates' labels [P], rl: the top-k's labels [KMAX].
  const bool carry = GROUPS && !GBIG && labels != nullptr;
  int* const cl = s_pre[wave];
  int* const rl = s_pre[wave] + P;
  static_assert(!GROUPS || GBIG || P + KMAX <= SMAX + 1, "label scratch must fit the prefix array");
  bool carried = false;
  if constexpr (GBIG) {
    // M <= P filtered members (checked above): exact keys, one bitonic sort, the first k
    double rd[E];
    int ri[E];
#pragma unroll
    for (int r = 0; r < E; ++r) {
      const int j = r * 64 + lane;
      rd[r] = INFINITY;
      ri[r] = -1;
      if (j < M) cand(j, rd[r], ri[r]);
    }
    dmlp::wave_sync();  // every member id read before the sorted keys overwrite the arrays
    dmlp::wave_sort_keys<E>(rd, ri);
#pragma unroll
    for (int r = 0; r < E; ++r) {
      s_d[wave][r * 64 + lane] = rd[r];
      s_i[wave][r * 64 + lane] = ri[r];
    }
    dmlp::wave_sync();
    res_d = s_d[wave];
    res_i = s_i[wave];
  } else if (M <= P && k <= KMAX) {
    // rank select: keys are unique (distinct ids), so rank(i) = #{j : key_j < key_i} places
    // every member of the top-k directly at its sorted position.
    double* cd = s_d[wave];
    int* ci = s_i[wave];
    for (int j = lane; j < M; j += 64) {
      double dv; int id;
      cand(j, dv, id);
      if (carry) cl[j] = labels[id];
      cd[j] = dv;
      if (!GROUPS) ci[j] = id;
    }
    carried = carry;
    for (int i = lane; i < k; i += 64) { s_rd[wave][i] = INFINITY; s_ri[wave][i] = -1; }
    dmlp::wave_sync();
    int Ms = M;
    if (M > 64 && k <= 64) {
      // O(M^2) ranking is the cost when the screen hands over a few hundred ids (4-row group
      // mode): the k-th smallest key of ANY subset bounds the k-th smallest of all from above,
      // so rank the first 64 candidates, keep only keys <= that bound (always >= k of them,
      // every true top-k member among them), and rank the survivors.
      const double di = cd[lane];
      const int ii = ci[lane];
      int rank = 0;
#pragma unroll 32
      for (int j = 0; j < 64; ++j) rank += dmlp::key_less(cd[j], ci[j], di, ii) ? 1 : 0;
      const unsigned long long hit = __ballot(rank == k - 1);
      const int src = __ffsll((long long)hit) - 1;
      const double td = __shfl(di, src);
      const int ti = __shfl(ii, src);
      dmlp::wave_sync();
      int kept = 0;
      for (int j0 = 0; j0 < M; j0 += 64) {
        const int j = j0 + lane;
        double dj = INFINITY;
        int ij = -1, lj = 0;
        bool keep = false;
        if (j < M) {
          dj = cd[j];
          ij = ci[j];
          if (carry) lj = cl[j];
          keep = !dmlp::key_less(td, ti, dj, ij);  // key_j <= bound
        }
        const unsigned long long km = __ballot(keep);
        dmlp::wave_sync();  // slots < j0 + 64 already read by every lane
        if (keep) {
          const int pos = kept + __popcll(km & dmlp::lanemask_lt());
          cd[pos] = dj;
          ci[pos] = ij;
          if (carry) cl[pos] = lj;
        }
        kept += __popcll(km);
      }
      dmlp::wave_sync();
      Ms = kept;
    }
    for (int i = lane; i < Ms; i += 64) {
      const double di = cd[i];
      const int ii = ci[i];
      int rank = 0;
#pragma unroll 32
      for (int j = 0; j < Ms; ++j) rank += dmlp::key_less(cd[j], ci[j], di, ii) ? 1 : 0;
      if (rank < k) {
        s_rd[wave][rank] = di;
        s_ri[wave][rank] = ii;
        if (carry) rl[rank] = cl[i];
      }
    }
    dmlp::wave_sync();
    res_d = s_rd[wave];
    res_i = s_ri[wave];
  } else {
    RunTopK<E> tk;
    tk.init(s_d[wave], s_i[wave], k);
    for (int j0 = 0; j0 < M; j0 += 64) {
      const int j = j0 + lane;
      const bool valid = j < M;
      int id = 0;
      double dv = INFINITY;
      if (valid) cand(j, dv, id);
      tk.push(valid, dv, id);
    }
    tk.flush();
    res_d = tk.d;
    res_i = tk.id;
  }
  for (int i = lane; i < k; i += 64) {
    out_d[(int64_t)q * kstride + i] = res_d[i];
    out_i[(int64_t)q * kstride + i] = res_i[i];
  }
  if (labels) {
    dmlp::wave_sync();
    if (carried) {
      const int label = k > 0 ? dmlp::wave_vote_by(res_i, k, [&](int i, int) { return rl[i]; },
                                                   label_lo, label_hi, s_hist[wave], HCAP)
                              : -1;
      if (lane == 0) {
        out_label[q] = label;
        out_cs[q] = dmlp::fnv_checksum(label, res_i, k);
      }
    } else {
      finalize_wave(res_i, k, labels, label_lo, label_hi, s_hist[wave], out_label + q,
                    out_cs + q, HCAP);
    }
  }
}

__global__ __launch_bounds__(256) void k_finalize(const double* __restrict__ d,
                                                  const int* __restrict__ ids, int kstride,
                                                  const int* __restrict__ qk,
                                                  const int* __restrict__ qidx, int nq,
                                                  const int* __restrict__ labels, int label_lo,
                                                  int label_hi, int* __restrict__ out_label,
                                                  uint64_t* __restrict__ out_cs) {
  __shared__ int s_hist[4][kHistCap];
  const int wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= nq) return;
  const int q = qidx ? qidx[i] : i;
  const int k = qk[q];
  finalize_wave(ids + (int64_t)q * kstride, k, labels, label_lo, label_hi, s_hist[wave],
                out_label + q, out_cs + q);
}

}  // namespace

extern "C" int dmlp_refine(int cap, const int* cand_ids, const int* cand_cnt, int S,
                           const double* X, int A, const double* Qx, const int* qidx,
                           const int* qk, int nq, double* out_d, int* out_i, int kstride,
                           const int* labels, int label_lo, int label_hi, int* out_label,
                           uint64_t* out_cs, int* status, int* ovf_count, void* stream) {
  if (nq <= 0) return 0;
  if (S < 1 || S > 256) return -1;
  const dim3 grid((nq + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  // cap is only the id stride per (query, slice).  P = 256 slots cover k + 64 for every k of the
  // cap <= 256 screens (<= 128); a larger P would cut the resident waves that hide the
  // row-gather latency, so only the cap-512 screen (128 < k <= 256) takes P = 512
  if (cap < 1) return -2;
  if (cap > 256)
    hipLaunchKernelGGL((k_refine<8, 0>), grid, block, 0, st, cand_ids, cand_cnt, S, cap, X, A,
                       Qx, qidx, qk, nq, out_d, out_i, kstride, labels, label_lo, label_hi,
                       out_label, out_cs, status, ovf_count, GroupIn{});
  else
    hipLaunchKernelGGL((k_refine<4, 0>), grid, block, 0, st, cand_ids, cand_cnt, S, cap, X, A,
                       Qx, qidx, qk, nq, out_d, out_i, kstride, labels, label_lo, label_hi,
                       out_label, out_cs, status, ovf_count, GroupIn{});
  DMLP_LAUNCH_CHECK();
  return 0;
}

static int refine_groups_impl(int cap, const int* cand_ids, const int* cand_cnt,
                              const float* cand_h, int S, const double* X, int A, const double* Qx,
                              const void* xfrag, const void* xrow, const float* xinit,
                              const void* qhi, int KT, int hl, int64_t n_points, const int* qidx,
                              const int* qk, int nq, double* out_d, int* out_i, int kstride,
                              const int* labels, int label_lo, int label_hi, int* out_label,
                              uint64_t* out_cs, int* status, int* ovf_count, int collect,
                              void* stream, int kmax = 64, int grows = 4,
                              const int* Xi = nullptr, const int* Qi = nullptr) {
  if (nq <= 0) return 0;
  if (grows != 4 && grows != 8) return -1;
  if (S < 1 || S > 256 || cap < 1 || n_points > 0x7fffffff) return -1;
  if (KT != 1 && KT != 2 && KT != 4 && KT != 8) return -1;
  if (hl != 1 && hl != 2) return -1;
  const int64_t n_tiles = (n_points + 63) / 64;
  GroupIn gin{cand_h, (const u32x4*)xfrag, xinit, (const bf16x8*)qhi, KT, hl, (int)n_points,
              (int)((n_tiles + S - 1) / S), collect ? 1 : 0};
  gin.grows = collect ? 4 : grows;
  gin.xi32 = Xi;
  // collect (the large-k lists, fp16 host operands only): k <= 256 over <= 512 filtered members
  if (collect) {
    if (hl != 1) return -1;
#define DMLP_REFINE_GB(KTV)                                                                    \
  hipLaunchKernelGGL((k_refine<8, KTV, true>), dim3((nq + 3) / 4), dim3(256), 0, (hipStream_t)stream, \
                     cand_ids, cand_cnt, S, cap, X, A, Qx, qidx, qk, nq, out_d, out_i, kstride, \
                     labels, label_lo, label_hi, out_label, out_cs, status, ovf_count, gin)
    if (KT == 1) DMLP_REFINE_GB(1);
    else if (KT == 2) DMLP_REFINE_GB(2);
    else if (KT == 4) DMLP_REFINE_GB(4);
    else DMLP_REFINE_GB(8);
#undef DMLP_REFINE_GB
    DMLP_LAUNCH_CHECK();
    return 0;
  }
  // one slice of the host's fp16 operands, k <= 32, labels: two queries per wave
  // (k_refine_pair; DMLP_REFINE_PAIR=0: the one-query-per-wave kernel).  Its PM = 64 member slots
  // leave >= 32 of slack above k only for k <= 32: at k near 64 any member inside the 2-eps band
  // would hand the query back, so the class k in (32, 64] takes k_refine (P = 128 slots)
  if (dmlp_refine_pair_path(S, hl, KT, labels != nullptr, cap, kmax)) {
    const dmlp::PairRefineArgs pa{cand_ids, cand_cnt, cap, cand_h, X, A, Qx, Xi, Qi, qidx, qk, nq,
                                  (const u32x4*)xfrag, (const u32x4*)xrow, xinit,
                                  (const bf16x8*)qhi, (int)n_points, out_d, out_i, kstride, labels,
                                  out_label, out_cs, status, ovf_count, gin.grows};
    dmlp::launch_refine_pair(KT, pa, (hipStream_t)stream);
    DMLP_LAUNCH_CHECK();
    return 0;
  }
  if ((!X && !Xi) || !Qx) return -3;  // (the other refines read fp64 queries)
#define DMLP_REFINE_G(KTV, F16)                                                                \
  hipLaunchKernelGGL((k_refine<2, KTV, F16>), dim3((nq + 3) / 4), dim3(256), 0, (hipStream_t)stream, \
                     cand_ids, cand_cnt, S, cap, X, A, Qx, qidx, qk, nq, out_d, out_i, kstride, \
                     labels, label_lo, label_hi, out_label, out_cs, status, ovf_count, gin)
  if (KT == 1) {
    if (hl == 1) DMLP_REFINE_G(1, true);
    else DMLP_REFINE_G(1, false);
  } else if (KT == 2) {
    if (hl == 1) DMLP_REFINE_G(2, true);
    else DMLP_REFINE_G(2, false);
  } else if (KT == 4) {
    if (hl == 1) DMLP_REFINE_G(4, true);
    else DMLP_REFINE_G(4, false);
  } else {
    if (hl == 1) DMLP_REFINE_G(8, true);
    else DMLP_REFINE_G(8, false);
  }
#undef DMLP_REFINE_G
  DMLP_LAUNCH_CHECK();
  return 0;
}

// The exact path's fp64 screen (screen_f64.hip): group ids of 4-point groups in slices of
// tiles_per_slice 64-point tiles, no rescoring image — every member of a group at or above the
// global threshold is re-ranked exactly (<= 512 members, k <= 256: the E = 8 variant).  Writes
// out_d / out_i only (no vote).
extern "C" int dmlp_refine_groups_exact(int cap, const int* cand_ids, const int* cand_cnt,
                                        const float* cand_h, int S, int64_t tiles_per_slice,
                                        const double* X, int A, const double* Qx, int64_t n_points,
                                        const int* qidx, const int* qk, int nq, double* out_d,
                                        int* out_i, int kstride, int* status, int* ovf_count,
                                        void* stream) {
  if (nq <= 0) return 0;
  if (S < 1 || S > 256 || cap < 1 || n_points > 0x7fffffff || tiles_per_slice < 1) return -1;
  GroupIn gin{cand_h, nullptr, nullptr, nullptr, 1, 1, (int)n_points, (int)tiles_per_slice, 0};
  gin.rescore = 0;
  hipLaunchKernelGGL((k_refine<8, 1, true>), dim3((nq + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                     cand_ids, cand_cnt, S, cap, X, A, Qx, qidx, qk, nq, out_d, out_i, kstride,
                     nullptr, 0, 1, nullptr, nullptr, status, ovf_count, gin);
  DMLP_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmlp_refine_groups2(int cap, const int* cand_ids, const int* cand_cnt,
                                   const float* cand_h, int S, const double* X, int A,
                                   const double* Qx, const void* xfrag, const float* xinit,
                                   const void* qhi, int KT, int hl, int64_t n_points,
                                   const int* qidx, const int* qk, int nq, double* out_d,
                                   int* out_i, int kstride, const int* labels, int label_lo,
                                   int label_hi, int* out_label, uint64_t* out_cs, int* status,
                                   int* ovf_count, int collect, void* stream) {
  // rows per group entry as the producing screen wrote them, told by its cap: the 16-entry
  // screen's id stride (dmlp_screen_x1_cap_kt(KT, 1)) means its groups, any other the 32-entry
  // screen's; the COLLECT pass always writes 4-row groups
  const int grows = collect ? 4
                    : cap == dmlp_screen_x1_cap_kt(KT, 1) ? dmlp_screen_x1_group_rows_kt(KT, 1)
                                                          : dmlp_screen_x1_group_rows_kt(KT, 64);
  return refine_groups_impl(cap, cand_ids, cand_cnt, cand_h, S, X, A, Qx, xfrag, nullptr, xinit,
                            qhi, KT, hl, n_points, qidx, qk, nq, out_d, out_i, kstride, labels,
                            label_lo, label_hi, out_label, out_cs, status, ovf_count, collect,
                            stream, 64, grows);
}

extern "C" int dmlp_refine_groups_rm(int cap, const int* cand_ids, const int* cand_cnt,
                                     const float* cand_h, int S, const double* X, int A,
                                     const double* Qx, const void* xfrag, const void* xrow,
                                     const float* xinit, const void* qhi, int KT, int hl,
                                     int64_t n_points, const int* qidx, const int* qk, int nq,
                                     double* out_d, int* out_i, int kstride, const int* labels,
                                     int label_lo, int label_hi, int* out_label, uint64_t* out_cs,
                                     int* status, int* ovf_count, int kmax, const int* Xi,
                                     const int* Qi, void* stream) {
  return refine_groups_impl(cap, cand_ids, cand_cnt, cand_h, S, X, A, Qx, xfrag, xrow, xinit, qhi,
                            KT, hl, n_points, qidx, qk, nq, out_d, out_i, kstride, labels,
                            label_lo, label_hi, out_label, out_cs, status, ovf_count, 0, stream,
                            kmax, dmlp_screen_x1_group_rows_kt(KT, kmax), Xi, Qi);
}

// Whether refine_groups_impl serves these lists with k_refine_pair: one slice of the host's fp16
// operands (S = 1, hl = 1, KT <= 2), labels, k <= 32 (PM = 64 member slots leave >= 32 of slack
// above k only there: at k near 64 any member inside the 2-eps band would hand the query back,
// so the class k in (32, 64] takes k_refine, P = 128 slots).  DMLP_REFINE_PAIR=0: never.  The
// pair refine also reads lossless int32 rows (dmlp_refine_groups_rm Xi / Qi), the others fp64.
extern "C" int dmlp_refine_pair_path(int S, int hl, int KT, int labels, int cap, int kmax) {
  static const bool pair_on = !(getenv("DMLP_REFINE_PAIR") && getenv("DMLP_REFINE_PAIR")[0] == '0');
  return pair_on && S == 1 && hl == 1 && KT <= 2 && labels && cap <= 128 && kmax <= 32 ? 1 : 0;
}

extern "C" int dmlp_refine_groups(int cap, const int* cand_ids, const int* cand_cnt,
                                  const float* cand_h, int S, const double* X, int A,
                                  const double* Qx, const void* xfrag, const float* xinit,
                                  const void* qhi, int KT, int hl, int64_t n_points, const int* qidx,
                                  const int* qk, int nq, double* out_d, int* out_i, int kstride,
                                  const int* labels, int label_lo, int label_hi, int* out_label,
                                  uint64_t* out_cs, int* status, int* ovf_count, void* stream) {
  return dmlp_refine_groups2(cap, cand_ids, cand_cnt, cand_h, S, X, A, Qx, xfrag, xinit, qhi, KT,
                             hl, n_points, qidx, qk, nq, out_d, out_i, kstride, labels, label_lo,
                             label_hi, out_label, out_cs, status, ovf_count, 0, stream);
}

extern "C" int dmlp_finalize(const double* d, const int* ids, int kstride, const int* qk,
                             const int* qidx, int nq, const int* labels, int label_lo, int label_hi, int* out_label,
                             uint64_t* out_cs, void* stream) {
  if (nq <= 0) return 0;
  hipLaunchKernelGGL(k_finalize, dim3((nq + 3) / 4), dim3(256), 0, (hipStream_t)stream, d, ids,
                     kstride, qk, qidx, nq, labels, label_lo, label_hi, out_label, out_cs);
  DMLP_LAUNCH_CHECK();
  return 0;
}
