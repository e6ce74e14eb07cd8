// report.hip — the report's lines, "Query <id> checksum: <u64>\n" (common.cpp:70), rendered on
// the GPU: k_fmt_len (line lengths, block-local scan), k_fmt_scan_blocks (block offsets),
// k_fmt_write (text through LDS, dword stores; the target may be page-locked host memory).
#include "dmlp.h"
#include "dmlp_device.h"

#include <algorithm>

namespace {

// ---- report formatting: "Query <qid> checksum: <cs>\n"
__device__ __forceinline__ int ndig_u64(uint64_t v) {
  int n = 1;
  while (v >= 10) { v /= 10; ++n; }
  return n;
}
__device__ __forceinline__ int line_len(int64_t qid, uint64_t cs) {
  return 6 + ndig_u64((uint64_t)qid) + 11 + ndig_u64(cs) + 1;
}

template <int FB>
__global__ void __launch_bounds__(FB) k_fmt_len(const uint64_t* __restrict__ cs, int nq,
                                                int qid_base, int64_t* __restrict__ off,
                                                int64_t* __restrict__ blocksum) {
  __shared__ int64_t sh[FB];
  const int i = blockIdx.x * FB + threadIdx.x;
  const int64_t v = i < nq ? line_len((int64_t)qid_base + i, cs[i]) : 0;
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < FB; o <<= 1) {  // inclusive Hillis-Steele scan
    const int64_t t = threadIdx.x >= (unsigned)o ? sh[threadIdx.x - o] : 0;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  if (i < nq) off[i + 1] = sh[threadIdx.x];  // block-local inclusive
  if (threadIdx.x == FB - 1) blocksum[blockIdx.x] = sh[FB - 1];
}

// Exclusive scan of the block sums in place (+ the total at [nb]): one 1024-thread block,
// 1024 sums per LDS pass with a running carry (a single-thread loop cost ~15 us at 128 blocks —
// one dependent global round trip per block).
__global__ void __launch_bounds__(1024) k_fmt_scan_blocks(int64_t* __restrict__ blocksum, int nb) {
  __shared__ int64_t sh[1024];
  int64_t carry = 0;
  for (int c0 = 0; c0 < nb; c0 += 1024) {
    const int b = c0 + (int)threadIdx.x;
    const int64_t v = b < nb ? blocksum[b] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive Hillis-Steele scan
      const int64_t t = threadIdx.x >= (unsigned)o ? sh[threadIdx.x - o] : 0;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    if (b < nb) blocksum[b] = carry + sh[threadIdx.x] - v;  // exclusive
    carry += sh[1023];
    __syncthreads();  // sh is rewritten by the next pass
  }
  if (threadIdx.x == 0) blocksum[nb] = carry;
}

// decimal digits of v written backwards so that the last one lands at txt[end - 1]: two 64-bit
// divisions by 1e9 at most, then 32-bit digit extraction (no per-digit 64-bit division, no
// dynamically indexed scratch buffer)
__device__ __forceinline__ void put_dec(char* txt, int end, uint64_t v) {
  int p = end;
  while (v >= 1000000000ull) {
    const uint64_t q = v / 1000000000ull;
    uint32_t r = (uint32_t)(v - q * 1000000000ull);
#pragma unroll
    for (int d = 0; d < 9; ++d) {
      txt[--p] = (char)('0' + r % 10u);
      r /= 10u;
    }
    v = q;
  }
  uint32_t r = (uint32_t)v;
  do {
    txt[--p] = (char)('0' + r % 10u);
    r /= 10u;
  } while (r);
}

// Each block renders its FB lines into LDS, then stores the block's byte range with dword
// stores (bytes only at the two unaligned ends).  The target may be page-locked host memory
// (the native engine writes the report straight into its output buffer): wide, contiguous
// stores keep the link busy where per-character stores would not.
template <int FB>
__global__ void __launch_bounds__(FB) k_fmt_write(const uint64_t* __restrict__ cs, int nq,
                                                 int qid_base, int64_t* __restrict__ off,
                                                 const int64_t* __restrict__ blocksum,
                                                 const int64_t* __restrict__ base,
                                                 char* __restrict__ out) {
  __shared__ char txt[FB * 48 + 4];
  const int i = blockIdx.x * FB + threadIdx.x;
  const int64_t b0 = base ? *base : 0;  // byte offset of this run's first line in out
  const int64_t g0 = b0 + blocksum[blockIdx.x], g1 = b0 + blocksum[blockIdx.x + 1];
  if (i < nq) {
    const int64_t qid = (int64_t)qid_base + i;
    const uint64_t v = cs[i];
    const int len = line_len(qid, v);
    const int64_t endl = off[i + 1];  // block-local inclusive end
    int pos = (int)(endl - len);
    const char* pre = "Query ";
    for (int c = 0; c < 6; ++c) txt[pos++] = pre[c];
    pos += ndig_u64((uint64_t)qid);
    put_dec(txt, pos, (uint64_t)qid);
    const char* mid = " checksum: ";
    for (int c = 0; c < 11; ++c) txt[pos++] = mid[c];
    pos += ndig_u64(v);
    put_dec(txt, pos, v);
    txt[pos++] = '\n';
  }
  __syncthreads();
  const int64_t a0 = (g0 + 3) & ~int64_t(3), a1 = std::max(a0, g1 & ~int64_t(3));
  if (threadIdx.x < 3) {  // unaligned head / tail bytes
    const int64_t h = g0 + threadIdx.x, tl = a1 + threadIdx.x;
    if (h < a0 && h < g1) out[h] = txt[h - g0];
    if (tl < g1 && tl >= a0) out[tl] = txt[tl - g0];
  }
  unsigned* o32 = reinterpret_cast<unsigned*>(out + a0);
  const int nw = (int)((a1 - a0) >> 2), b = (int)(a0 - g0);
  for (int w = threadIdx.x; w < nw; w += FB) {
    const int s = b + 4 * w;
    o32[w] = (unsigned)(unsigned char)txt[s] | ((unsigned)(unsigned char)txt[s + 1] << 8) |
             ((unsigned)(unsigned char)txt[s + 2] << 16) |
             ((unsigned)(unsigned char)txt[s + 3] << 24);
  }
  if (i < nq) off[i + 1] += g0;
  if (i == 0) off[0] = b0;
}

// lines per format block: 256 (512 blocks for the headline's 131072 lines push the report's
// PCIe writes from more CUs than 1024-line blocks: 106.5 vs 109.4 us, profiles/r12k_fmt_block_ab.txt)
constexpr int kFmtBlock = 256;

}  // namespace

extern "C" int64_t dmlp_format_bound(int nq) { return (int64_t)nq * 48 + 64; }

// line_off needs nq + 1 + (nq/FB + 2) int64 of scratch; on completion line_off[nq] = bytes.
extern "C" int64_t dmlp_format_scratch(int nq) {
  return (int64_t)nq + 1 + (nq + kFmtBlock - 1) / kFmtBlock + 1;
}

extern "C" int dmlp_format_report(const uint64_t* cs, int nq, int qid_base, int64_t* line_off,
                                  char* out, void* stream) {
  return dmlp_format_report_at(cs, nq, qid_base, line_off, out, nullptr, stream);
}

// The same, the lines starting at byte *base of out (device word; null: 0): a report rendered in
// query parts, each part's base = the previous part's line_off[nq] (its absolute end).
// k_fmt_write aligns its dword stores on the byte offset in out, not on the address: out must be
// 4-byte aligned (-1 before any launch otherwise, like dmlp_rows_from_i32's operands).
extern "C" int dmlp_format_report_at(const uint64_t* cs, int nq, int qid_base, int64_t* line_off,
                                     char* out, const int64_t* base, void* stream) {
  if (nq <= 0) return 0;
  if ((uintptr_t)out & 3) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (nq + kFmtBlock - 1) / kFmtBlock;
  int64_t* blocksum = line_off + nq + 1;
  hipLaunchKernelGGL(k_fmt_len<kFmtBlock>, dim3(nb), dim3(kFmtBlock), 0, st, cs, nq, qid_base,
                     line_off, blocksum);
  DMLP_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_fmt_scan_blocks, dim3(1), dim3(1024), 0, st, blocksum, nb);
  DMLP_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_fmt_write<kFmtBlock>, dim3(nb), dim3(kFmtBlock), 0, st, cs, nq, qid_base,
                     line_off, blocksum, base, out);
  DMLP_LAUNCH_CHECK();
  return 0;
}
