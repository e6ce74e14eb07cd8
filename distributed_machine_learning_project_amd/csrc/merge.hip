// merge.hip — K-way merge of sorted per-shard top-k lists (K4) and two list utilities.
//
//  * dmlp_merge : the device analog of bench_2's user MPI_Op (@0xbc70) and bench_1's root
//                 sort (@0xdae6); RCCL has no user reductions, so strategies call this between
//                 send/recv rounds.  L <= 8 lists: k_merge_win / k_merge_seq (one lane per
//                 query, heads in registers); more: k_merge_path (LDS merge path) or the rank
//                 kernel k_merge.
//  * dmlp_offset_ids, dmlp_fill_f64 : shard-local -> global ids, and a constant fill.
#include "dmlp.h"
#include "dmlp_device.h"
#include <float.h>

#include <algorithm>

namespace {

// K-way merge of L sorted top-k lists per query (K4: bench_2's custom MPI_Op / bench_1's root
// merge), one wave per query, no sequential head scan: every element's output position is its
// rank in the union, i.e. its index in its own list plus, for every other list, the number of
// entries ordered before it (a binary search over that list's real prefix; ties between lists
// go to the lower list index).  The ranks of the real elements are therefore exactly
// 0 .. total-1; each element with rank < k is stored once, and slots [min(total, k), kout) get
// the (+inf, -1) padding.  Padding entries (id < 0) form a suffix of each list.
__global__ __launch_bounds__(256) void k_merge(const double* __restrict__ in_d,
                                               const int* __restrict__ in_i, int L,
                                               int64_t list_stride, int kin,
                                               const int* __restrict__ qk, int nq,
                                               double* __restrict__ out_d, int* __restrict__ out_i,
                                               int kout) {
  __shared__ int s_cnt[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + wave;
  if (q >= nq) return;
  int k = qk[q];
  k = k < kout ? k : kout;
  k = k > 0 ? k : 0;
  const int lim = k < kin ? k : kin;
  const int64_t qo = (int64_t)q * kin;
  int* cnt = s_cnt[wave];
  // real prefix length of each list (first padding entry, by binary search)
  for (int l = lane; l < L; l += 64) {
    const int* ids = in_i + l * list_stride + qo;
    int lo = 0, n = lim;
    while (n > 0) {
      const int h = n >> 1;
      if (ids[lo + h] >= 0) { lo += h + 1; n -= h + 1; } else { n = h; }
    }
    cnt[l] = lo;
  }
  dmlp::wave_sync();
  int total = 0;
  for (int l = 0; l < L; ++l) total += cnt[l];
  for (int t = lane; t < L * lim; t += 64) {
    const int l = t / lim, p = t - l * lim;
    if (p >= cnt[l]) continue;
    const int64_t off = l * list_stride + qo + p;
    const double d = in_d[off];
    const int id = in_i[off];
    int rank = p;
    for (int m = 0; m < L && rank < k; ++m) {
      if (m == l) continue;
      const double* md = in_d + m * list_stride + qo;
      const int* mi = in_i + m * list_stride + qo;
      // equal keys (only when the caller's lists overlap) order by list index, as a sequential
      // merge that scans the lists in order would: count entries <= the key in earlier lists
      const bool before = m < l;
      int lo = 0, n = cnt[m];
      while (n > 0) {
        const int h = n >> 1;
        const bool lt = before ? !dmlp::key_less(d, id, md[lo + h], mi[lo + h])
                               : dmlp::key_less(md[lo + h], mi[lo + h], d, id);
        if (lt) { lo += h + 1; n -= h + 1; } else { n = h; }
      }
      rank += lo;
    }
    if (rank < k) {
      out_d[(int64_t)q * kout + rank] = d;
      out_i[(int64_t)q * kout + rank] = id;
    }
  }
  // every slot past the merged entries, up to kout, is padding (as in the L <= 8 kernels)
  for (int o = (total < k ? total : k) + lane; o < kout; o += 64) {
    out_d[(int64_t)q * kout + o] = INFINITY;
    out_i[(int64_t)q * kout + o] = -1;
  }
}

// Merge-path form of the same K4 merge for lists that fit in LDS (2 x L x kout entries):
// one wave per query stages the L real prefixes in LDS, then merges adjacent pairs level by
// level (log2 L levels, ties to the lower list index, i.e. the earlier pair member — the same
// order as the rank kernel).  Every output element of a pair merge finds its co-rank (how many
// of its predecessors come from the first list) by one binary search, so a lane does
// ceil(pairs x k / 64) searches of log2 k probes per level, all in LDS.
__global__ __launch_bounds__(256) void k_merge_path(const double* __restrict__ in_d,
                                                   const int* __restrict__ in_i, int L,
                                                   int64_t list_stride, int kin,
                                                   const int* __restrict__ qk, int nq,
                                                   double* __restrict__ out_d,
                                                   int* __restrict__ out_i, int kout, int lcap) {
  extern __shared__ __attribute__((aligned(16))) char smem_all[];
  __shared__ int s_cnt_all[4][2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * (blockDim.x >> 6) + wave;  // one query per wave
  if (q >= nq) return;
  char* const smem = smem_all + (size_t)wave * 2 * L * lcap * (sizeof(double) + sizeof(int));
  int (*s_cnt)[64] = s_cnt_all[wave];
  int k = qk[q];
  k = k < kout ? k : kout;
  k = k > 0 ? k : 0;
  const int lim = k < kin ? k : kin;
  double* bd[2] = {(double*)smem, (double*)smem + (size_t)L * lcap};
  int* bi[2] = {(int*)((double*)smem + 2 * (size_t)L * lcap),
                (int*)((double*)smem + 2 * (size_t)L * lcap) + (size_t)L * lcap};
  const int64_t qo = (int64_t)q * kin;
  // t / d for the small flat indices below by a float reciprocal (exact: t < 2^16, +0.5 margin)
  auto divq = [](int t, float inv) { return (int)(((float)t + 0.5f) * inv); };
  // stage the L prefixes (all loads of a lane issued back to back), then each list's real
  // prefix length by a binary search for its first padding id
  const float inv_lim = 1.0f / (float)(lim > 0 ? lim : 1);
  for (int t0 = 0; t0 < L * lim; t0 += 256) {  // 4 loads in flight per lane, then the stores
    double dv[4];
    int iv[4], dst[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = t0 + 64 * u + lane;
      dst[u] = -1;
      if (t < L * lim) {
        const int l = divq(t, inv_lim), p = t - l * lim;
        const int64_t off = l * list_stride + qo + p;
        dv[u] = in_d[off];
        iv[u] = in_i[off];
        dst[u] = l * lcap + p;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (dst[u] >= 0) { bd[0][dst[u]] = dv[u]; bi[0][dst[u]] = iv[u]; }
  }
  dmlp::wave_sync();
  for (int l = lane; l < L; l += 64) {
    const int* ids = bi[0] + l * lcap;
    int lo = 0, n = lim;
    while (n > 0) {
      const int h = n >> 1;
      if (ids[lo + h] >= 0) { lo += h + 1; n -= h + 1; } else { n = h; }
    }
    s_cnt[0][l] = lo;
  }
  dmlp::wave_sync();
  const float inv_k = 1.0f / (float)(k > 0 ? k : 1);
  int cur = 0, Lc = L;
  while (Lc > 1) {
    const int Ln = (Lc + 1) >> 1;
    const double* sd = bd[cur];
    const int* si = bi[cur];
    double* dd = bd[cur ^ 1];
    int* di = bi[cur ^ 1];
    // lane-contiguous output ranges over the flattened (pair, position) space: one co-rank
    // search per pair segment, then a sequential merge of the segment from register heads
    const int tot = Ln * k;
    const int chunk = (tot + 63) >> 6;
    int t = lane * chunk;
    const int tend = t + chunk < tot ? t + chunk : tot;
    while (t < tend) {
      const int pr = divq(t, inv_k), o0 = t - pr * k;
      const int oend = o0 + (tend - t) < k ? o0 + (tend - t) : k;
      t += oend - o0;
      const int la = 2 * pr, lb = la + 1;
      const int ca = s_cnt[cur][la];
      const double* ad = sd + la * lcap;
      const int* ai = si + la * lcap;
      double* od = dd + pr * lcap;
      int* oi = di + pr * lcap;
      if (lb >= Lc) {
        for (int o = o0; o < oend && o < ca; ++o) { od[o] = ad[o]; oi[o] = ai[o]; }
        continue;
      }
      const int cb = s_cnt[cur][lb];
      const int m = ca + cb < oend ? ca + cb : oend;
      if (o0 >= m) continue;
      const double* b_d = sd + lb * lcap;
      const int* b_i = si + lb * lcap;
      // co-rank of o0: the smallest i with NOT (a[i] precedes b[o0 - i - 1]); a first on ties
      int lo = o0 > cb ? o0 - cb : 0, hi = o0 < ca ? o0 : ca;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int j = o0 - mid - 1;
        if (!dmlp::key_less(b_d[j], b_i[j], ad[mid], ai[mid])) lo = mid + 1; else hi = mid;
      }
      int i = lo, j = o0 - lo;
      double xa = i < ca ? ad[i] : 0.0, xb = j < cb ? b_d[j] : 0.0;
      int ia = i < ca ? ai[i] : 0, ib = j < cb ? b_i[j] : 0;
      for (int o = o0; o < m; ++o) {
        const bool take_a = i < ca && (j >= cb || !dmlp::key_less(xb, ib, xa, ia));
        if (take_a) {
          od[o] = xa; oi[o] = ia;
          if (++i < ca) { xa = ad[i]; ia = ai[i]; }
        } else {
          od[o] = xb; oi[o] = ib;
          if (++j < cb) { xb = b_d[j]; ib = b_i[j]; }
        }
      }
    }
    if (lane < Ln) {
      const int la = 2 * lane, lb = la + 1;
      const int c = s_cnt[cur][la] + (lb < Lc ? s_cnt[cur][lb] : 0);
      s_cnt[cur ^ 1][lane] = c < k ? c : k;
    }
    dmlp::wave_sync();
    cur ^= 1;
    Lc = Ln;
  }
  const int total = s_cnt[cur][0];  // <= k
  for (int o = lane; o < kout; o += 64) {  // real entries, then padding up to kout
    const bool real = o < total;
    out_d[(int64_t)q * kout + o] = real ? bd[cur][o] : INFINITY;
    out_i[(int64_t)q * kout + o] = real ? bi[cur][o] : -1;
  }
}

// Register-resident sequential form for few lists (L <= 8): one LANE per query, the L list
// heads in registers, one output per iteration (the smallest head under (dist asc, id desc);
// equal keys go to the lower list index: a later list must be strictly smaller to win), then
// one load refills the list it came from.  No LDS, no co-rank searches, no wave-wide
// synchronisation: 64 queries per wave, and the per-query work is k selections of L heads —
// the merge-path kernel spends a whole wave per query.  Padding entries (id < 0) end a list;
// slots [total, kout) get the (+inf, -1) padding, so callers need no fill pass.
template <int L>
__global__ __launch_bounds__(256) void k_merge_seq(const double* __restrict__ in_d,
                                                  const int* __restrict__ in_i,
                                                  int64_t list_stride, int kin,
                                                  const int* __restrict__ qk, int nq,
                                                  double* __restrict__ out_d,
                                                  int* __restrict__ out_i, int kout) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  int k = qk[q];
  k = k < kout ? k : kout;
  k = k > 0 ? k : 0;
  const int lim = k < kin ? k : kin;
  const int64_t qo = (int64_t)q * kin;
  double hd[L];
  int hi[L], pos[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    pos[l] = 0;
    hd[l] = INFINITY;
    hi[l] = -1;
    if (lim > 0) {
      hd[l] = in_d[l * list_stride + qo];
      hi[l] = in_i[l * list_stride + qo];
    }
  }
  double* const od = out_d + (int64_t)q * kout;
  int* const oi = out_i + (int64_t)q * kout;
  int o = 0;
  for (; o < k; ++o) {
    int b = -1;
    double bd = INFINITY;
    int bi = -1;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const bool better = hi[l] >= 0 && (b < 0 || dmlp::key_less(hd[l], hi[l], bd, bi));
      b = better ? l : b;
      bd = better ? hd[l] : bd;
      bi = better ? hi[l] : bi;
    }
    if (b < 0) break;  // every list exhausted
    od[o] = bd;
    oi[o] = bi;
    int pb = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) pb = l == b ? pos[l] : pb;
    ++pb;
    double nd = INFINITY;
    int ni = -1;
    if (pb < lim) {
      const int64_t off = b * list_stride + qo + pb;
      nd = in_d[off];
      ni = in_i[off];
    }
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const bool t = l == b;
      pos[l] = t ? pb : pos[l];
      hd[l] = t ? nd : hd[l];
      hi[l] = t ? ni : hi[l];
    }
  }
  for (; o < kout; ++o) {
    od[o] = INFINITY;
    oi[o] = -1;
  }
}

// Windowed form of k_merge_seq for lists whose length is a multiple of 4 (16-byte aligned
// rows): each list's next 4 entries sit in registers as a shift window (the head is always
// slot 0), filled by one 32-byte + one 16-byte load per list up front and refilled only when a
// list has given 4 outputs.  For k = 16 over 8 lists most queries never refill, so the per-lane
// chain of dependent loads (one per output in k_merge_seq) collapses to the initial fill, and
// the cache-line requests drop by 3/4 (4 entries per request instead of 1).
template <int L>
__global__ __launch_bounds__(256) void k_merge_win(const double* __restrict__ in_d,
                                                  const int* __restrict__ in_i,
                                                  int64_t list_stride, int kin,
                                                  const int* __restrict__ qk, int nq,
                                                  double* __restrict__ out_d,
                                                  int* __restrict__ out_i, int kout) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  int k = qk[q];
  k = k < kout ? k : kout;
  k = k > 0 ? k : 0;
  const int lim = k < kin ? k : kin;
  const int64_t qo = (int64_t)q * kin;
  double wd[L][4];
  int wi[L][4];
  int nxt[L];  // list position of the entry after the window
  auto fill = [&](int l, int p, double (&d)[4], int (&id)[4]) __attribute__((always_inline)) {
    const int64_t off = l * list_stride + qo + p;
    const double2 a = *(const double2*)(in_d + off);
    const double2 b = *(const double2*)(in_d + off + 2);
    const int4 c = *(const int4*)(in_i + off);
    d[0] = a.x; d[1] = a.y; d[2] = b.x; d[3] = b.y;
    // entries at or past lim end the list (the id < 0 test below)
    id[0] = p < lim ? c.x : -1;
    id[1] = p + 1 < lim ? c.y : -1;
    id[2] = p + 2 < lim ? c.z : -1;
    id[3] = p + 3 < lim ? c.w : -1;
  };
#pragma unroll
  for (int l = 0; l < L; ++l) {
    nxt[l] = 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) { wd[l][j] = INFINITY; wi[l][j] = -1; }
    if (lim > 0) fill(l, 0, wd[l], wi[l]);
  }
  double* const od = out_d + (int64_t)q * kout;
  int* const oi = out_i + (int64_t)q * kout;
  int o = 0;
  for (; o < k; ++o) {
    int b = -1;
    double bd = INFINITY;
    int bi = -1;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const bool better = wi[l][0] >= 0 && (b < 0 || dmlp::key_less(wd[l][0], wi[l][0], bd, bi));
      b = better ? l : b;
      bd = better ? wd[l][0] : bd;
      bi = better ? wi[l][0] : bi;
    }
    if (b < 0) break;  // every list exhausted
    od[o] = bd;
    oi[o] = bi;
    // shift list b's window; refill it when its last entry was just taken
    bool refill = false;
    int rp = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      if (l == b) {
        wd[l][0] = wd[l][1]; wd[l][1] = wd[l][2]; wd[l][2] = wd[l][3]; wd[l][3] = INFINITY;
        wi[l][0] = wi[l][1]; wi[l][1] = wi[l][2]; wi[l][2] = wi[l][3]; wi[l][3] = -1;
        refill = wi[l][0] < 0 && nxt[l] < lim;
        rp = nxt[l];
      }
    }
    if (refill) {
      double nd[4];
      int ni[4];
      fill(b, rp, nd, ni);
#pragma unroll
      for (int l = 0; l < L; ++l) {
        if (l == b) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { wd[l][j] = nd[j]; wi[l][j] = ni[j]; }
          nxt[l] += 4;
        }
      }
    }
  }
  for (; o < kout; ++o) {
    od[o] = INFINITY;
    oi[o] = -1;
  }
}

__global__ void k_fill_f64(double* __restrict__ p, int64_t n, double v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = v;
}

__global__ void k_offset_ids(int* __restrict__ ids, int64_t n, int off) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    if (ids[i] >= 0) ids[i] += off;
}

}  // namespace

extern "C" int dmlp_merge(const double* in_d, const int* in_i, int L, int64_t list_stride,
                          int kin, const int* qk, int nq, double* out_d, int* out_i, int kout,
                          void* stream) {
  if (nq <= 0) return 0;
  if (L < 1 || L > 64) return -1;
  const int lcap = std::max(1, kout);  // a merged list holds up to k <= kout entries
  const size_t lds = 2 * (size_t)L * lcap * (sizeof(double) + sizeof(int));
  if (L <= 8) {  // one lane per query, heads in registers (writes every slot of [0, kout))
    const dim3 g((nq + 255) / 256), b(256);
    hipStream_t st = (hipStream_t)stream;
    // 16-byte window loads: every list start (l * list_stride + q * kin) must be 4-aligned too
    const bool win = kin % 4 == 0 && list_stride % 4 == 0 && ((uintptr_t)in_d & 15) == 0 &&
                     ((uintptr_t)in_i & 15) == 0 &&
                     !(getenv("DMLP_MERGE_WIN") && getenv("DMLP_MERGE_WIN")[0] == '0');
    if (win) {
#define DMLP_MERGE_WIN(LV)                                                                     \
  case LV:                                                                                     \
    hipLaunchKernelGGL(k_merge_win<LV>, g, b, 0, st, in_d, in_i, list_stride, kin, qk, nq, out_d, \
                       out_i, kout);                                                           \
    break;
      switch (L) {
        DMLP_MERGE_WIN(1) DMLP_MERGE_WIN(2) DMLP_MERGE_WIN(3) DMLP_MERGE_WIN(4)
        DMLP_MERGE_WIN(5) DMLP_MERGE_WIN(6) DMLP_MERGE_WIN(7) DMLP_MERGE_WIN(8)
      }
#undef DMLP_MERGE_WIN
      DMLP_LAUNCH_CHECK();
      return 0;
    }
#define DMLP_MERGE_SEQ(LV)                                                                     \
  case LV:                                                                                     \
    hipLaunchKernelGGL(k_merge_seq<LV>, g, b, 0, st, in_d, in_i, list_stride, kin, qk, nq, out_d, \
                       out_i, kout);                                                           \
    break;
    switch (L) {
      DMLP_MERGE_SEQ(1) DMLP_MERGE_SEQ(2) DMLP_MERGE_SEQ(3) DMLP_MERGE_SEQ(4)
      DMLP_MERGE_SEQ(5) DMLP_MERGE_SEQ(6) DMLP_MERGE_SEQ(7) DMLP_MERGE_SEQ(8)
    }
#undef DMLP_MERGE_SEQ
  } else if (lds <= 48 * 1024) {  // LDS-resident merge path (P <= 8 lists of k <= 256, ...)
    const int w = lds <= 12 * 1024 ? 4 : 1;  // queries (waves) per workgroup
    hipLaunchKernelGGL(k_merge_path, dim3((nq + w - 1) / w), dim3(64 * w), lds * w,
                       (hipStream_t)stream, in_d, in_i, L, list_stride, kin, qk, nq, out_d, out_i,
                       kout, lcap);
  } else {
    hipLaunchKernelGGL(k_merge, dim3((nq + 3) / 4), dim3(256), 0, (hipStream_t)stream, in_d,
                       in_i, L, list_stride, kin, qk, nq, out_d, out_i, kout);
  }
  DMLP_LAUNCH_CHECK();
  return 0;
}

// shard-local ids -> global ids (padding -1 kept)
extern "C" int dmlp_offset_ids(int* ids, int64_t n, int off, void* stream) {
  if (n <= 0 || off == 0) return 0;
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(k_offset_ids, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ids,
                     n, off);
  DMLP_LAUNCH_CHECK();
  return 0;
}

extern "C" int dmlp_fill_f64(double* p, int64_t n, double v, void* stream) {
  if (n <= 0) return 0;
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(k_fill_f64, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, n,
                     v);
  DMLP_LAUNCH_CHECK();
  return 0;
}
