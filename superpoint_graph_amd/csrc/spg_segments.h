// Internal interface of the segment kernels (spg_segments.hip): PointNet above 128 points per superpoint.
//
// A superpoint of P > 128 points is cut into S = P / Ps segments of Ps points (Ps: the largest divisor of P that is <= 128, at
// least 32).  The convolutions of a stack run on B * S pseudo-superpoints of Ps points -- the row space [B * P] is the same, row
// b * P + p = (b * S + s) * Ps + p' -- and only three things are per superpoint: the cloud layout, the 2 x 2 transform and the
// max-pool.  These kernels translate them between the two views; plain vector loads and stores, no atomics.
#pragma once
#include "spg_common.h"

#define SPG_SEG_MIN_PS 32
#define SPG_SEG_NPTS_END 4096      // sizes from here on are refused (the size queries have always refused 4096)
// the rule as one sentence, for the error messages of the library
#define SPG_SEG_RULE "npts must be in [1, 128], or in (128, 4096) with a divisor in [32, 128] (the largest one is the segment length: " \
                     "256 = 2 x 128, 160 = 2 x 80, 1000 = 8 x 125; 131 and 262 have none)"

// false: npts outside the supported set
inline bool spg_segment_plan(int P, int* Ps, int* S) {
  if (P >= 1 && P <= 128) { *Ps = P; *S = 1; return true; }
  if (P >= SPG_SEG_NPTS_END) return false;
  for (int d = 128; d >= SPG_SEG_MIN_PS; --d)
    if (P % d == 0) { *Ps = d; *S = P / d; return true; }
  return false;
}

// seg [B * S, nfeat, Ps] = clouds [B, nfeat, P], P = S * Ps: segment s of superpoint b holds its points s * Ps ... (s + 1) * Ps - 1
int spg_launch_segment_clouds(const float* clouds, int B, int nfeat, int P, int Ps, float* seg, hipStream_t stream);
// segT [B * S, 4] = T [B, 4], every row S times (the raw projection of the inner STN, or an external transform)
int spg_launch_segment_transforms(const float* T, int B, int S, float* segT, hipStream_t stream);
// Max-pool over the S segments of a superpoint.  spool / sidx [B * S, ldseg]: the value each segment selected (max, or min where
// sign[c] < 0) and the point inside the segment that holds it (sidx may be null: no winners, inference through the convolution
// stack kernel).  pooled [B, ldpool]: min where sign[c] < 0, else max, by a strict comparison in ascending segment order -- the
// first extremum wins (torch's tie rule); aidx [B, ldpool]: its point index in 0 ... P - 1; pooled[b, C + e] = extra[b, e].
int spg_launch_pool_merge(const float* spool, const int* sidx, long ldseg, const float* sign, int B, int S, int Ps, int C,
                          const float* extra, int nextra, float* pooled, int* aidx, long ldpool, hipStream_t stream);
// The max-pool's backward in the segments' view: gseg [B * S, ldseg] = dpool[b, c] in the segment that holds the winner, else 0;
// lidx [B * S, ldseg] = the winner's point index inside that segment, else -1 (no row of the segment matches it)
int spg_launch_pool_expand(const float* dpool, const int* aidx, long ldpool, int B, int S, int Ps, int C, float* gseg, int* lidx,
                           long ldseg, hipStream_t stream);
// dT [B, 4] = sum over s = 0 ... S - 1, in that order, of dTseg [B * S, 4]
int spg_launch_segment_dT_sum(const float* dTseg, int B, int S, float* dT, hipStream_t stream);
