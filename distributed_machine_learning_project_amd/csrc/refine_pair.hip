// refine_pair.hip — the group refine at TWO queries per wave (k_refine_pair) and its launcher.
// refine.hip's refine_groups_impl picks it for the lists dmlp_refine_pair_path accepts.
#include "dmlp.h"
#include "dmlp_device.h"
#include "refine_common.h"
#include <float.h>

namespace {

// element i of a row table: the fp64 rows, or (Xi non-null) the lossless int32 rows divided back
// exactly as k_rows_from_i32 does (prep.hip: the host checked x == fl(m / 1e6) for every value)
__device__ __forceinline__ double row_value(const double* __restrict__ X, const int* __restrict__ Xi,
                                            int64_t i) {
  return Xi ? (double)Xi[i] / 1.0e6 : X[i];
}

// Group refine, TWO queries per wave (32 lanes each): the one-slice single-term screen on the
// host's fp16 operands (S = 1, hl = 1, KT <= 2), labels given; the kernel holds k <= 64, the host sends it k <= 32
// (dmlp_refine_pair_path: the slack above k in the PM member slots).  k_refine (one query per
// wave) is bound by its chain of dependent gathers — group entries -> member fragments -> exact
// rows -> labels — at 8 waves per SIMD, i.e. 8 queries in flight per SIMD; here each wave keeps
// two queries' chains in flight with about the same registers per lane.  Members are scored one
// per lane per batch (32 per query), so the usual ~72 members take 3 batches.  More than PM
// surviving members hand the query back (status 1, as k_refine does past its P).
//
// The shipped configuration, and what its measured alternatives cost:
//  * one member per lane per batch at 8 waves/SIMD (KT = 1): 239 us vs 289 us for 2 at 5, r7w
//    (U = 2 at 5 waves: 288 us; profiles/r7n_refine_ab.txt)
//  * 8 lanes per exact row in the survivors' phase: 8 (218 us), 16 (239 us, r8c) or 4 (222 us, r12p)
//  * member scores by v_dot2c_f32_f16 (219 -> 212 us, 0 spills; r8h), not cvt + fma
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
template <int KT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KT == 1 ? 8 : 4))) void k_refine_pair(
    const int* __restrict__ cand_ids, const int* __restrict__ cand_cnt, int cap,
    const float* __restrict__ cand_h, const double* __restrict__ X, int A,
    const double* __restrict__ Qx, const int* __restrict__ Xi, const int* __restrict__ Qi,
    const int* __restrict__ qidx, const int* __restrict__ qk,
    int nq, const u32x4* __restrict__ xfrag, const u32x4* __restrict__ xrow,
    const float* __restrict__ xinit, const bf16x8* __restrict__ qhi, int n_points,
    double* __restrict__ out_d, int* __restrict__ out_i, int kstride,
    const int* __restrict__ labels, int* __restrict__ out_label, uint64_t* __restrict__ out_cs,
    int* __restrict__ status, int* __restrict__ ovf_count, int grows) {
  constexpr int PM = 64;   // surviving members per query
  constexpr int KM = 64;   // top-k slots per query (the host admits k <= 32)
  constexpr int EC = 4;    // group entries held per lane (cap <= 128)
  __shared__ int s_i[8][PM];
  __shared__ double s_d[8][PM];
  __shared__ int s_l[8][PM];
  __shared__ double s_rd[8][KM];
  __shared__ int s_ri[8][KM];
  __shared__ int s_rl[8][KM];
  __shared__ __attribute__((aligned(16))) unsigned s_qh[8][16 * KT];  // hi(q') as fp16 pairs
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, hl = lane & 31;
  const int slot = wave * 2 + half;
  const int p = blockIdx.x * 8 + slot;
  bool act = p < nq;
  const int q = act ? (qidx ? qidx[p] : p) : 0;
  const int k = act ? qk[q] : 0;
  const int n = act ? cand_cnt[p] : 0;
  const float hq = act ? cand_h[2 * (int64_t)p] : 0.0f;
  unsigned ent[EC];
#pragma unroll
  for (int u = 0; u < EC; ++u) {
    const int j = hl + 32 * u;
    ent[u] = act && j < n && j < cap ? (unsigned)cand_ids[(int64_t)p * cap + j] : 0u;
  }
  // hi(q') in LDS, read at each use (held in registers it pushed the kernel into spills)
  {
    const unsigned short* qh = (const unsigned short*)(qhi + (int64_t)q * KT * 4);
    for (int a = hl; a < 16 * KT; a += 32)
      s_qh[slot][a] = act ? (unsigned)qh[2 * a] | ((unsigned)qh[2 * a + 1] << 16) : 0u;
  }
  if (act)
    for (int i = k + hl; i < kstride; i += 32) {
      out_d[(int64_t)q * kstride + i] = INFINITY;
      out_i[(int64_t)q * kstride + i] = -1;
    }
  if (act && n < 0) {
    if (hl == 0) {
      status[q] = 1;
      if (ovf_count) atomicAdd(ovf_count, 1);
    }
    act = false;
  } else if (act && hl == 0) {
    status[q] = 0;
  }
  const int M = act ? n : 0;
  const unsigned tq = __float_as_uint(hq);
  const unsigned kh = (tq ^ ((unsigned)((int)tq >> 31) | 0x80000000u)) & 0xffff0000u;
  // ---- members: one per lane per batch; keep those whose single-term score reaches hq
  int Mw = M;  // wave-uniform trip count: the larger half's
  Mw = max(Mw, __shfl_xor(Mw, 32));
  int nm = 0;
  dmlp::wave_sync();  // s_qh written
  const int GS = grows == 8 ? 3 : 2;  // members per group entry, log2
  for (int j0 = 0; j0 < (Mw << GS); j0 += 32) {
    __asm__ volatile("" ::: "memory");  // keep the s_qh reads in the loop
    const int jm = j0 + hl;
    const int g = jm >> GS;
    const int src = half * 32 + (g & 31);
    unsigned e = 0;
#pragma unroll
    for (int c = 0; c < EC; ++c) {
      const unsigned v = (unsigned)__shfl((int)ent[c], src);
      if ((g >> 5) == c) e = v;
    }
    const int id = dmlp::group_row(e & 0xffffu, jm & (grows - 1), grows);
    const bool pass = g < M && e >= kh && id < n_points;
    const int pt = pass ? id : 0;
    u32x4 w[KT * 4];
    if (xrow) {  // the point's 64 * KT bytes in one run (k_x1_rowmajor): one line per member
      const u32x4* fr = xrow + (int64_t)pt * (4 * KT);
#pragma unroll
      for (int f = 0; f < 4 * KT; ++f)
        w[f] = pass ? fr[f] : u32x4{0, 0, 0, 0};
    } else {
      const u32x4* fr = xfrag + (int64_t)(pt >> 6) * (4 * KT * 64) + (pt & 15);
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int kq = 0; kq < 4; ++kq)
          w[kt * 4 + kq] = pass ? fr[(int64_t)((((pt & 63) >> 4) * KT + kt) * 64) + 16 * kq]
                                : u32x4{0, 0, 0, 0};
    }
    float sc = pass ? xinit[pt] : 0.0f;
#pragma unroll
    for (int f = 0; f < KT * 4; ++f) {
      // v_dot2c_f32_f16: two exact fp16 products added into the fp32 score per instruction (at
      // most two roundings per pair, A in all: inside the screen bound like the MFMA's chain;
      // fp16 subnormal inputs are not flushed: tools/probe/dot2_probe.hip).  The words are taken
      // out of the vectors first: w[f][q2] inside the builtin's operand compiled to word 0
      // of each fragment for every q2 (one dword load per fragment, wrong scores)
      const uint4 qv = *(const uint4*)&s_qh[slot][4 * f];
      const u32x4 xv = w[f];
      const unsigned qw[4] = {qv.x, qv.y, qv.z, qv.w};
      const unsigned xw[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
      for (int q2 = 0; q2 < 4; ++q2)
        sc = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2v, qw[q2]),
                                    __builtin_bit_cast(f16x2v, xw[q2]), sc, false);
    }
    const bool keep = pass && sc >= hq;
    const unsigned long long bm = __ballot(keep);
    const unsigned hm = (unsigned)(bm >> (32 * half));
    const int pos = nm + __popc(hm & ((1u << hl) - 1u));
    if (keep && pos < PM) s_i[slot][pos] = id;
    nm += __popc(hm);
  }
  if (act && nm > PM) {  // pathological ties: hand the query back
    if (hl == 0) {
      status[q] = 1;
      if (ovf_count) atomicAdd(ovf_count, 1);
    }
    act = false;
  }
  const int Ms = act ? nm : 0;
  dmlp::wave_sync();
  // ---- exact distances of the survivors in the reference's order (engine.cpp:12-18), 8 lanes
  // per row (four rows per round): lane t holds attributes E t .. E t + E-1 (+ 32 u) of the row —
  // a row is read by a few wide loads, where a lane-per-row gather touched a line per lane per
  // load (the rows were half of this kernel's time: profiles/r7m_refine_ablation.txt) — squares
  // their differences (each product rounded, no FMA), adds its E products to its predecessor's
  // partial sum in order, and the sum moves on by a DPP row shift, so the last lane ends with
  // exactly the reference's sum (fewer rounds and chain steps than 16 lanes per row)
  {
    constexpr int RL = 8, E = 32 / RL;
    const int t8 = hl & (RL - 1), rsel = hl / RL;
    double qa[KT][E];
#pragma unroll
    for (int u = 0; u < KT; ++u)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int a = 32 * u + E * t8 + e;
        qa[u][e] = a < A ? row_value(Qx, Qi, (int64_t)q * A + a) : 0.0;
      }
    int Msw = Ms;
    Msw = max(Msw, __shfl_xor(Msw, 32));
    for (int r0 = 0; r0 < Msw; r0 += 32 / RL) {
      const int j = r0 + rsel;
      const bool rv = j < Ms;
      const int id = rv ? s_i[slot][j] : 0;
      const int64_t xb = (int64_t)id * A;
      double pr[KT][E];
#pragma unroll
      for (int u = 0; u < KT; ++u) {
        const int a0 = 32 * u + E * t8;
        double x[E];
        if (Xi && rv && a0 + E - 1 < A && (A & 3) == 0) {
          // lossless int32 rows: half the bytes of the gather (one 16-byte load per 4 values),
          // each value divided back exactly as k_rows_from_i32 does
#pragma unroll
          for (int e = 0; e < E; e += 4) {
            const int4 v = *(const int4*)(Xi + xb + a0 + e);
            x[e] = (double)v.x / 1.0e6;
            x[e + 1] = (double)v.y / 1.0e6;
            x[e + 2] = (double)v.z / 1.0e6;
            x[e + 3] = (double)v.w / 1.0e6;
          }
        } else if (!Xi && rv && a0 + E - 1 < A && (A & 1) == 0) {  // 16-byte pairs
#pragma unroll
          for (int e = 0; e < E; e += 2) {
            const double2 v = *(const double2*)(X + xb + a0 + e);
            x[e] = v.x;
            x[e + 1] = v.y;
          }
        } else {
#pragma unroll
          for (int e = 0; e < E; ++e)
            x[e] = rv && a0 + e < A ? row_value(X, Xi, xb + a0 + e) : 0.0;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double d = a0 + e < A ? __dsub_rn(qa[u][e], x[e]) : 0.0;
          pr[u][e] = __dmul_rn(d, d);
        }
      }
      double sm = 0.0;
#pragma unroll
      for (int u = 0; u < KT; ++u) {
        // lane 0 of the group continues from the last lane's total of the previous 32 attributes
        const double tl = u == 0 ? 0.0 : __shfl(sm, (lane & ~(RL - 1)) | (RL - 1));
#pragma unroll
        for (int t = 0; t < RL; ++t) {
          double in = tl;
          if (t > 0) {
            const long long b = __double_as_longlong(sm);
            const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0x111, 0xf, 0xf, false);
            const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x111, 0xf, 0xf, false);
            in = __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
          }
          double v = in;
#pragma unroll
          for (int e = 0; e < E; ++e) v = __dadd_rn(v, pr[u][e]);
          sm = t8 == t ? v : sm;
        }
      }
      if (rv && t8 == RL - 1) {
        s_d[slot][j] = sm;
        s_l[slot][j] = labels[id];
      }
    }
  }
  for (int i = hl; i < KM; i += 32) {
    s_rd[slot][i] = INFINITY;
    s_ri[slot][i] = -1;
    s_rl[slot][i] = 0;
  }
  dmlp::wave_sync();
  // ---- rank select: keys are unique, rank = #{ keys before } places the top-k directly
  for (int j = hl; j < Ms; j += 32) {
    const double dj = s_d[slot][j];
    const int ij = s_i[slot][j];
    int r = 0;
    for (int i = 0; i < Ms; ++i) r += dmlp::key_less(s_d[slot][i], s_i[slot][i], dj, ij) ? 1 : 0;
    if (r < k) {
      s_rd[slot][r] = dj;
      s_ri[slot][r] = ij;
      s_rl[slot][r] = s_l[slot][j];
    }
  }
  dmlp::wave_sync();
  if (act)
    for (int i = hl; i < k; i += 32) {
      out_d[(int64_t)q * kstride + i] = s_rd[slot][i];
      out_i[(int64_t)q * kstride + i] = s_ri[slot][i];
    }
  // ---- vote (max count, tie -> larger label; padding ids < 0 not counted) + FNV checksum
  long long best = -1;
  for (int i = hl; i < k; i += 32) {
    if (s_ri[slot][i] < 0) continue;
    const int li = s_rl[slot][i];
    int c = 0;
    for (int j = 0; j < k; ++j) c += (s_ri[slot][j] >= 0 && s_rl[slot][j] == li) ? 1 : 0;
    const long long key = ((long long)c << 32) | (long long)((unsigned)li ^ 0x80000000u);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) {
    const long long o = __shfl_xor(best, off);
    best = o > best ? o : best;
  }
  if (act && hl == 0) {
    const int label = best < 0 ? -1 : (int)((unsigned)(best & 0xffffffffll) ^ 0x80000000u);
    out_label[q] = label;
    out_cs[q] = dmlp::fnv_checksum(label, s_ri[slot], k);
  }
}

}  // namespace

void dmlp::launch_refine_pair(int KT, const PairRefineArgs& a, hipStream_t stream) {
  auto kern = KT == 1 ? k_refine_pair<1> : k_refine_pair<2>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((a.nq + 7) / 8)), dim3(256), 0, stream, a.cand_ids,
                     a.cand_cnt, a.cap, a.cand_h, a.X, a.A, a.Qx, a.Xi, a.Qi, a.qidx, a.qk, a.nq,
                     a.xfrag, a.xrow, a.xinit, a.qhi, a.n_points, a.out_d, a.out_i, a.kstride,
                     a.labels, a.out_label, a.out_cs, a.status, a.ovf_count, a.grows);
}
