// Weighted cross entropy over the superpoint logits (learning/main.py:205: nn.functional.cross_entropy(outputs,
// label_mode, weight=class_weights), ignore_index = -100) as ONE forward and ONE backward launch: log-softmax, the
// weighted negative log-likelihood, its normaliser and the gradient wrt the logits.  N is a few thousand rows of <= 64
// classes: one workgroup, fixed summation order (deterministic).  torch needs five launches for the same.
#include "../../include/spg_hip.h"
#include "spg_common.h"

namespace {

__global__ __launch_bounds__(1024) void ce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                      const float* __restrict__ weight, int N, int C, int64_t ignore_index,
                                                      int reduction_mean, float* __restrict__ loss, float* __restrict__ lse,
                                                      float* __restrict__ wsum_out) {
  __shared__ double s_l[16], s_w[16];
  __shared__ int s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  double accl = 0.0, accw = 0.0;
  for (int i = threadIdx.x; i < N; i += 1024) {
    const float* x = logits + (long)i * C;
    float m = -FLT_MAX;
    for (int c = 0; c < C; ++c) m = fmaxf(m, x[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(x[c] - m);
    const float ls = logf(s);
    lse[i] = m + ls;
    const int64_t t = target[i];
    if (t != ignore_index && t >= 0 && t < C) {
      const float w = weight ? weight[t] : 1.f;
      accl += (double)(w * (ls - (x[t] - m)));      // nll = log s - (x_t - m): m + log s rounds at |m| >> 1 and would cancel here
      accw += (double)w;
    } else if (t != ignore_index) {
      s_bad = 1;      // a class index outside [0, C) that is not ignore_index: torch raises a device assert; here the loss becomes NaN
    }
  }
  for (int off = 32; off >= 1; off >>= 1) { accl += __shfl_xor(accl, off, 64); accw += __shfl_xor(accw, off, 64); }
  if ((threadIdx.x & 63) == 0) { s_l[threadIdx.x >> 6] = accl; s_w[threadIdx.x >> 6] = accw; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int k = 0; k < 16; ++k) { a += s_l[k]; b += s_w[k]; }
    *wsum_out = (float)b;
    *loss = s_bad ? __builtin_nanf("") : (float)(reduction_mean ? a / b : a);
  }
}

__global__ void ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target, const float* __restrict__ weight,
                              const float* __restrict__ wsum, const float* __restrict__ grad_loss,
                              int N, int C, int64_t ignore_index, int reduction_mean, float* __restrict__ grad_logits) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)N * C) return;
  const int i = (int)(idx / C), c = (int)(idx - (long)i * C);
  const int64_t t = target[i];
  float g = 0.f;
  if (t != ignore_index && t >= 0 && t < C) {
    // softmax = exp((x - m) - log s) with the row's maximum and sum formed again by the forward's own loops (C <= 64 values):
    // the stored lse = m + log s is rounded at the magnitude of m, an absolute error of ulp(m) / 2 in the exponent -- 5e-4
    // RELATIVE in every gradient of a row whose logits sit at 1e4 (tests/test_gpu_op_edges.py).
    const float* x = logits + (long)i * C;
    float m = -FLT_MAX;
    for (int k = 0; k < C; ++k) m = fmaxf(m, x[k]);
    float s = 0.f;
    for (int k = 0; k < C; ++k) s += expf(x[k] - m);
    const float w = weight ? weight[t] : 1.f;
    const float scale = (*grad_loss) * w / (reduction_mean ? *wsum : 1.f);
    g = scale * (expf((x[c] - m) - logf(s)) - (c == (int)t ? 1.f : 0.f));
  }
  grad_logits[idx] = g;
}

// forward and backward in ONE launch (the gradient of the loss itself is 1): workgroup 0 is the forward kernel above (loss,
// log-sum-exp per row, normaliser); every further workgroup takes CE_ROWS rows of the gradient -- it re-derives what it needs
// from the forward with the forward's own arithmetic and summation order (the normaliser over all rows, the log-sum-exp of
// its rows), so loss and gradient are bit-identical to the two separate launches.  (A single workgroup doing both took 20 us
// against 8.5 + 4.7 for the pair: the 13 000 gradient elements behind the forward's critical path.)
#define CE_ROWS 64
__global__ __launch_bounds__(1024) void ce_fwd_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                          const float* __restrict__ weight, int N, int C, int64_t ignore_index,
                                                          int reduction_mean, float* __restrict__ loss, float* __restrict__ lse,
                                                          float* __restrict__ wsum_out, float* __restrict__ grad_logits) {
  __shared__ double s_l[16], s_w[16];
  __shared__ int s_bad;
  __shared__ float s_wsum;
  __shared__ float s_max[CE_ROWS], s_logsum[CE_ROWS];
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    double accl = 0.0, accw = 0.0;
    for (int i = threadIdx.x; i < N; i += 1024) {
      const float* x = logits + (long)i * C;
      float m = -FLT_MAX;
      for (int c = 0; c < C; ++c) m = fmaxf(m, x[c]);
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += expf(x[c] - m);
      const float ls = logf(s);
      lse[i] = m + ls;
      const int64_t t = target[i];
      if (t != ignore_index && t >= 0 && t < C) {
        const float w = weight ? weight[t] : 1.f;
        accl += (double)(w * (ls - (x[t] - m)));
        accw += (double)w;
      } else if (t != ignore_index) {
        s_bad = 1;
      }
    }
    for (int off = 32; off >= 1; off >>= 1) { accl += __shfl_xor(accl, off, 64); accw += __shfl_xor(accw, off, 64); }
    if ((threadIdx.x & 63) == 0) { s_l[threadIdx.x >> 6] = accl; s_w[threadIdx.x >> 6] = accw; }
    __syncthreads();
    if (threadIdx.x == 0) {
      double a = 0.0, b = 0.0;
      for (int k = 0; k < 16; ++k) { a += s_l[k]; b += s_w[k]; }
      *wsum_out = (float)b;
      *loss = s_bad ? __builtin_nanf("") : (float)(reduction_mean ? a / b : a);
    }
    return;
  }
  // ---- gradient rows [r0, r1) ----
  const int r0 = ((int)blockIdx.x - 1) * CE_ROWS, r1 = min(N, r0 + CE_ROWS);
  float wsum = 1.f;
  if (reduction_mean) {      // the normaliser, summed exactly like workgroup 0 sums it
    double accw = 0.0;
    for (int i = threadIdx.x; i < N; i += 1024) {
      const int64_t t = target[i];
      if (t != ignore_index && t >= 0 && t < C) accw += (double)(weight ? weight[t] : 1.f);
    }
    for (int off = 32; off >= 1; off >>= 1) accw += __shfl_xor(accw, off, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = accw;
    __syncthreads();
    if (threadIdx.x == 0) {
      double b = 0.0;
      for (int k = 0; k < 16; ++k) b += s_w[k];
      s_wsum = (float)b;
    }
  }
  if ((int)threadIdx.x < r1 - r0) {
    const float* x = logits + (long)(r0 + threadIdx.x) * C;
    float m = -FLT_MAX;
    for (int c = 0; c < C; ++c) m = fmaxf(m, x[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(x[c] - m);
    s_max[threadIdx.x] = m;
    s_logsum[threadIdx.x] = logf(s);
  }
  __syncthreads();
  if (reduction_mean) wsum = s_wsum;
  for (int e = threadIdx.x; e < (r1 - r0) * C; e += 1024) {
    const int il = e / C, c = e - il * C;
    const long idx = (long)(r0 + il) * C + c;
    const int64_t t = target[r0 + il];
    float g = 0.f;
    if (t != ignore_index && t >= 0 && t < C) {
      const float w = weight ? weight[t] : 1.f;
      const float scale = 1.f * w / (reduction_mean ? wsum : 1.f);
      g = scale * (expf((logits[idx] - s_max[il]) - s_logsum[il]) - (c == (int)t ? 1.f : 0.f));
    }
    grad_logits[idx] = g;
  }
}

}  // namespace

extern "C" int spg_cross_entropy_fwd_bwd(const float* logits, const int64_t* target, const float* weight, int N, int C,
                                         int64_t ignore_index, int reduction_mean, float* loss, float* lse, float* wsum,
                                         float* grad_logits, void* stream) {
  SPG_CHECK_ARG(logits && target && loss && lse && wsum && grad_logits && N > 0 && C > 0, "bad argument");
  hipLaunchKernelGGL(ce_fwd_bwd_kernel, dim3(1 + spg_cdiv(N, CE_ROWS)), dim3(1024), 0, (hipStream_t)stream, logits, target, weight, N, C,
                     ignore_index, reduction_mean, loss, lse, wsum, grad_logits);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_cross_entropy_fwd(const float* logits, const int64_t* target, const float* weight, int N, int C,
                                     int64_t ignore_index, int reduction_mean, float* loss, float* lse, float* wsum, void* stream) {
  SPG_CHECK_ARG(logits && target && loss && lse && wsum && N > 0 && C > 0, "bad argument");
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits, target, weight, N, C, ignore_index,
                     reduction_mean, loss, lse, wsum);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_cross_entropy_bwd(const float* logits, const int64_t* target, const float* weight, const float* lse,
                                     const float* wsum, const float* grad_loss, int N, int C, int64_t ignore_index,
                                     int reduction_mean, float* grad_logits, void* stream) {
  SPG_CHECK_ARG(logits && target && lse && wsum && grad_loss && grad_logits && N > 0 && C > 0, "bad argument");
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(spg_cdiv((long)N * C, 256)), dim3(256), 0, (hipStream_t)stream, logits, target, weight,
                     wsum, grad_loss, N, C, ignore_index, reduction_mean, grad_logits);      // (lse: an output of the forward, not read)
  SPG_LAUNCH_CHECK();
  return 0;
}
