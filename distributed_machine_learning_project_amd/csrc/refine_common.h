// refine_common.h — what refine.hip and refine_pair.hip share (internal: not part of dmlp.h).
#pragma once
#include "dmlp_device.h"

namespace dmlp {

// row of member i (< grows) of the group with slice-relative entry index gi
__device__ __forceinline__ int group_row(unsigned gi, int i, int grows) {
  return grows == 8 ? (int)(gi >> 2) * 32 + (int)(gi & 3) * 4 + ((i & 4) << 2) + (i & 3)
                    : (int)gi * 4 + i;
}

// k_refine_pair's arguments (refine_pair.hip), in the kernel's own order
struct PairRefineArgs {
  const int* cand_ids;
  const int* cand_cnt;
  int cap;
  const float* cand_h;
  const double* X;
  int A;
  const double* Qx;
  const int* Xi;  // lossless int32 rows / queries (X / Qx unused), or null
  const int* Qi;
  const int* qidx;
  const int* qk;
  int nq;
  const u32x4* xfrag;
  const u32x4* xrow;  // the image point-major (k_x1_rowmajor), or null
  const float* xinit;
  const bf16x8* qhi;
  int n_points;
  double* out_d;
  int* out_i;
  int kstride;
  const int* labels;
  int* out_label;
  uint64_t* out_cs;
  int* status;
  int* ovf_count;
  int grows;
};

// launches k_refine_pair<KT> (KT 1 or 2) over a.nq queries, 8 per block
void launch_refine_pair(int KT, const PairRefineArgs& a, hipStream_t stream);

}  // namespace dmlp
