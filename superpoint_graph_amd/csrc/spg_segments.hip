// PointNet above 128 points per superpoint: the kernels between the superpoints' view [B, P] and the segments' view [B * S, Ps]
// (spg_segments.h; the plan is made in spg_pointnet.hip).  Each is one thread per output element, bandwidth-bound and small next
// to the convolutions: the cloud copy moves 2 * nfeat * 4 bytes per point, the tables 8 bytes per (segment, channel).
#include "spg_segments.h"
#include <float.h>

namespace {

__global__ void segment_clouds_kernel(const float* __restrict__ clouds, long n, int nfeat, int P, int Ps, int S,
                                      float* __restrict__ seg) {
  const long o = (long)blockIdx.x * blockDim.x + threadIdx.x;      // = ((b * S + s) * nfeat + c) * Ps + p': coalesced on both sides
  if (o >= n) return;
  const long row = o / Ps;                 // (b * S + s) * nfeat + c
  const int pp = (int)(o - row * Ps);
  const long bs = row / nfeat;
  const int c = (int)(row - bs * nfeat);
  const long b = bs / S;
  const int s = (int)(bs - b * S);
  seg[o] = clouds[(b * nfeat + c) * P + (long)s * Ps + pp];
}

__global__ void segment_transforms_kernel(const float* __restrict__ T, long n, int S, float* __restrict__ segT) {
  const long o = (long)blockIdx.x * blockDim.x + threadIdx.x;      // = (b * S + s) * 4 + e
  if (o >= n) return;
  const long bs = o >> 2;
  segT[o] = T[(bs / S) * 4 + (o & 3)];
}

__global__ void pool_merge_kernel(const float* __restrict__ spool, const int* __restrict__ sidx, long ldseg,
                                  const float* __restrict__ sign, int B, int S, int Ps, int C, const float* __restrict__ extra,
                                  int nextra, float* __restrict__ pooled, int* __restrict__ aidx, long ldpool) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int W = C + nextra;
  if (i >= (long)B * W) return;
  const long b = i / W;
  const int c = (int)(i - b * W);
  if (c >= C) { pooled[b * ldpool + c] = extra[b * nextra + (c - C)]; return; }
  const bool down = sign != nullptr && sign[c] < 0.f;      // the rule of the convolution's epilogue: min where gamma < 0, else max
  const long r0 = b * S * ldseg + c;
  float best = spool[r0];
  int sb = 0;
  for (int s = 1; s < S; ++s) {      // ascending segments, strict comparison: the first extremum stays
    const float v = spool[r0 + s * ldseg];
    const bool better = down ? v < best : v > best;
    best = better ? v : best; sb = better ? s : sb;
  }
  pooled[b * ldpool + c] = best;
  if (aidx != nullptr && sidx != nullptr) aidx[b * ldpool + c] = sb * Ps + sidx[r0 + sb * ldseg];
}

__global__ void pool_expand_kernel(const float* __restrict__ dpool, const int* __restrict__ aidx, long ldpool, long n, int S,
                                   int Ps, int C, float* __restrict__ gseg, int* __restrict__ lidx, long ldseg) {
  const long o = (long)blockIdx.x * blockDim.x + threadIdx.x;      // = (b * S + s) * ldseg + c
  if (o >= n) return;
  const long bs = o / ldseg;
  const int c = (int)(o - bs * ldseg);
  const long b = bs / S;
  const int s = (int)(bs - b * S);
  float g = 0.f;
  int li = -1;
  if (c < C) {      // (the padding columns of a row are defined too: zero gradient, no winner)
    const int w = aidx[b * ldpool + c] - s * Ps;
    if (w >= 0 && w < Ps) { g = dpool[b * ldpool + c]; li = w; }
  }
  gseg[o] = g; lidx[o] = li;
}

__global__ void segment_dT_sum_kernel(const float* __restrict__ dTseg, long n, int S, float* __restrict__ dT) {
  const long o = (long)blockIdx.x * blockDim.x + threadIdx.x;      // = b * 4 + e
  if (o >= n) return;
  const long b = o >> 2;
  const int e = (int)(o & 3);
  float a = 0.f;
  for (int s = 0; s < S; ++s) a += dTseg[(b * S + s) * 4 + e];
  dT[o] = a;
}

}  // namespace

int spg_launch_segment_clouds(const float* clouds, int B, int nfeat, int P, int Ps, float* seg, hipStream_t stream) {
  SPG_CHECK_ARG(clouds && seg && B > 0 && nfeat > 0 && Ps > 0 && P % Ps == 0, "segment_clouds arguments");
  const long n = (long)B * nfeat * P;
  hipLaunchKernelGGL(segment_clouds_kernel, dim3(spg_cdiv(n, 256)), dim3(256), 0, stream, clouds, n, nfeat, P, Ps, P / Ps, seg);
  SPG_LAUNCH_CHECK();
  return 0;
}

int spg_launch_segment_transforms(const float* T, int B, int S, float* segT, hipStream_t stream) {
  SPG_CHECK_ARG(T && segT && B > 0 && S > 0, "segment_transforms arguments");
  const long n = (long)B * S * 4;
  hipLaunchKernelGGL(segment_transforms_kernel, dim3(spg_cdiv(n, 256)), dim3(256), 0, stream, T, n, S, segT);
  SPG_LAUNCH_CHECK();
  return 0;
}

int spg_launch_pool_merge(const float* spool, const int* sidx, long ldseg, const float* sign, int B, int S, int Ps, int C,
                          const float* extra, int nextra, float* pooled, int* aidx, long ldpool, hipStream_t stream) {
  SPG_CHECK_ARG(spool && pooled && B > 0 && S > 0 && Ps > 0 && C > 0 && ldseg >= C && ldpool >= C + nextra && (nextra == 0 || extra),
                "pool_merge arguments");
  const long n = (long)B * (C + nextra);
  hipLaunchKernelGGL(pool_merge_kernel, dim3(spg_cdiv(n, 256)), dim3(256), 0, stream, spool, sidx, ldseg, sign, B, S, Ps, C, extra,
                     nextra, pooled, aidx, ldpool);
  SPG_LAUNCH_CHECK();
  return 0;
}

int spg_launch_pool_expand(const float* dpool, const int* aidx, long ldpool, int B, int S, int Ps, int C, float* gseg, int* lidx,
                           long ldseg, hipStream_t stream) {
  SPG_CHECK_ARG(dpool && aidx && gseg && lidx && B > 0 && S > 0 && Ps > 0 && C > 0 && ldseg >= C && ldpool >= C, "pool_expand arguments");
  const long n = (long)B * S * ldseg;
  hipLaunchKernelGGL(pool_expand_kernel, dim3(spg_cdiv(n, 256)), dim3(256), 0, stream, dpool, aidx, ldpool, n, S, Ps, C, gseg, lidx,
                     ldseg);
  SPG_LAUNCH_CHECK();
  return 0;
}

int spg_launch_segment_dT_sum(const float* dTseg, int B, int S, float* dT, hipStream_t stream) {
  SPG_CHECK_ARG(dTseg && dT && B > 0 && S > 0, "segment_dT_sum arguments");
  const long n = (long)B * 4;
  hipLaunchKernelGGL(segment_dT_sum_kernel, dim3(spg_cdiv(n, 256)), dim3(256), 0, stream, dTseg, n, S, dT);
  SPG_LAUNCH_CHECK();
  return 0;
}
