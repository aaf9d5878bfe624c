// Edge-conditioned convolution + GRU kernels for gfx950 (reference: learning/ecc/GraphConvModule.py:44-152,
// learning/ecc/cuda_kernels.py:55-139, learning/modules.py:152-183,224-251).
//
// Design (MI355X-first, not a translation of the reference's one-thread-per-channel CUDA kernels):
//   * one 64-lane wavefront owns one graph node; the whole RNN-ECC iteration for that node
//     (gather x_src, per-edge 32x32 filter product, mean over the in-edges, input gate, the two
//     32->96 GRU projections, row normalisation, gates) is ONE kernel: the per-edge products and the
//     aggregate never exist in HBM;
//   * a 32x32 filter is read as 4 x 16-byte loads per lane (1 KiB per wave instruction, fully
//     coalesced); partial sums are reduced across lanes with wave shuffles once per node;
//   * no atomics anywhere: the backward walks a reverse CSR (by source) built once per batch, so
//     results are deterministic.
#include "spg_ecc.h"
#include <mutex>

// ---------------------------------------------------------------------------------------------
// graph build
// ---------------------------------------------------------------------------------------------
static inline size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

struct GraphLayout {
  size_t hdr, rowptr, src, dst, rev_eid, invdeg, rev_rowptr, cursor, total;
};
// target-side arrays first (their offsets depend on N and E only); the source-side arrays, whose length is
// the number of SOURCE rows Ns >= N (GraphConvFunction allows more input rows than output nodes), come last.
static GraphLayout graph_layout(int N, int Ns, int E) {
  GraphLayout L;
  size_t o = 0;
  L.hdr = o; o += 16;
  L.rowptr = o; o += al16((size_t)(N + 1) * 4);
  L.src = o; o += al16((size_t)(E + 1) * 4);
  L.dst = o; o += al16((size_t)(E + 1) * 4);
  L.rev_eid = o; o += al16((size_t)(E + 1) * 4);
  L.invdeg = o; o += al16((size_t)(N + 1) * 4);
  L.rev_rowptr = o; o += al16((size_t)(Ns + 1) * 4);
  L.cursor = o; o += al16((size_t)(Ns + 1) * 4);
  L.total = o;
  return L;
}
size_t spg_graph_bytes(int N, int Ns, int E) { return graph_layout(N, Ns < N ? N : Ns, E).total; }

SpgGraph spg_graph_view(const void* ws, int N, int E) {
  GraphLayout L = graph_layout(N, N, E);
  const char* b = (const char*)ws;
  SpgGraph g;
  g.N = N; g.E = E;
  g.hdr = (const int*)(b + L.hdr);
  g.rowptr = (const int*)(b + L.rowptr);
  g.src = (const int*)(b + L.src);
  g.dst = (const int*)(b + L.dst);
  g.rev_rowptr = (const int*)(b + L.rev_rowptr);
  g.rev_eid = (const int*)(b + L.rev_eid);
  g.invdeg = (const float*)(b + L.invdeg);
  return g;
}

template <typename TIn>
__global__ __launch_bounds__(1024) void spg_scan_kernel(const TIn* __restrict__ in, int n, int* __restrict__ out) {
  __shared__ long part[1024];
  const int t = threadIdx.x;
  const int chunk = (n + 1023) / 1024;
  const int b = min(n, t * chunk), e = min(n, b + chunk);
  long s = 0;
  for (int i = b; i < e; ++i) s += (long)in[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const long v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  long base = part[t] - s;
  for (int i = b; i < e; ++i) {
    out[i] = (int)base;
    base += (long)in[i];
  }
  if (t == 1023) out[n] = (int)part[1023];
}

__global__ void spg_graph_nodes_kernel(const int64_t* __restrict__ degs, const int* __restrict__ rowptr, int N, int Ns,
                                       int E, int* __restrict__ hdr, int* __restrict__ dst, float* __restrict__ invdeg,
                                       int* __restrict__ cursor) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { hdr[0] = N; hdr[1] = Ns; hdr[2] = E; hdr[3] = 0; }
  if (i < Ns) cursor[i] = 0;
  if (i >= N) return;
  const int d = (int)degs[i];
  invdeg[i] = d > 0 ? 1.0f / (float)d : 0.f;
  const int e0 = rowptr[i];
  for (int k = 0; k < d; ++k) dst[e0 + k] = i;
}

__global__ void spg_graph_edges_kernel(const int64_t* __restrict__ idxn, int E, int Ns, int* __restrict__ src,
                                       int* __restrict__ cnt, int* __restrict__ hdr) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int64_t j64 = idxn[e];
  if (j64 < 0 || j64 >= Ns) {   // malformed index buffer: flag it, never write out of bounds
    src[e] = 0;
    atomicOr(&hdr[3], 1);
    return;
  }
  const int j = (int)j64;
  src[e] = j;
  atomicAdd(&cnt[j], 1);   // integer count only: the result is order-independent
}

__global__ void spg_graph_revfill_kernel(const int* __restrict__ src, int E, const int* __restrict__ rev_rowptr,
                                         int* __restrict__ cursor, int* __restrict__ rev_eid) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int j = src[e];
  const int pos = atomicAdd(&cursor[j], 1);
  rev_eid[rev_rowptr[j] + pos] = e;
}

__global__ void spg_graph_revsort_kernel(const int* __restrict__ rev_rowptr, int N, int* __restrict__ rev_eid) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const int b = rev_rowptr[j], e = rev_rowptr[j + 1];
  for (int a = b + 1; a < e; ++a) {   // insertion sort: out-degrees are small
    const int v = rev_eid[a];
    int k = a - 1;
    while (k >= b && rev_eid[k] > v) { rev_eid[k + 1] = rev_eid[k]; --k; }
    rev_eid[k + 1] = v;
  }
}

int spg_graph_build_impl(const int64_t* idxn, const int64_t* degs, int N, int Ns, int E, void* ws, hipStream_t stream) {
  SPG_CHECK_ARG(N > 0 && E >= 0, "graph needs N > 0");
  if (Ns < N) Ns = N;
  GraphLayout L = graph_layout(N, Ns, E);
  char* b = (char*)ws;
  int* rowptr = (int*)(b + L.rowptr);
  int* src = (int*)(b + L.src);
  int* dst = (int*)(b + L.dst);
  int* rev_rowptr = (int*)(b + L.rev_rowptr);
  int* rev_eid = (int*)(b + L.rev_eid);
  float* invdeg = (float*)(b + L.invdeg);
  int* cursor = (int*)(b + L.cursor);
  int* hdr = (int*)(b + L.hdr);
  hipLaunchKernelGGL(spg_scan_kernel<int64_t>, dim3(1), dim3(1024), 0, stream, degs, N, rowptr);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(spg_graph_nodes_kernel, dim3(spg_cdiv(Ns, 256)), dim3(256), 0, stream, degs, rowptr, N, Ns, E, hdr, dst,
                     invdeg, cursor);
  SPG_LAUNCH_CHECK();
  if (E > 0) {
    hipLaunchKernelGGL(spg_graph_edges_kernel, dim3(spg_cdiv(E, 256)), dim3(256), 0, stream, idxn, E, Ns, src, cursor, hdr);
    SPG_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(spg_scan_kernel<int>, dim3(1), dim3(1024), 0, stream, (const int*)cursor, Ns, rev_rowptr);
  SPG_LAUNCH_CHECK();
  hipError_t me = hipMemsetAsync(cursor, 0, (size_t)Ns * 4, stream);
  if (me != hipSuccess) { spg_set_error("hipMemsetAsync failed: %s", hipGetErrorString(me)); return (int)me; }
  if (E > 0) {
    hipLaunchKernelGGL(spg_graph_revfill_kernel, dim3(spg_cdiv(E, 256)), dim3(256), 0, stream, (const int*)src, E,
                       (const int*)rev_rowptr, cursor, rev_eid);
    SPG_LAUNCH_CHECK();
    hipLaunchKernelGGL(spg_graph_revsort_kernel, dim3(spg_cdiv(Ns, 256)), dim3(256), 0, stream, (const int*)rev_rowptr, Ns,
                       rev_eid);
    SPG_LAUNCH_CHECK();
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float spg_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// Synchronisation point of the per-node helpers.  The per-iteration kernels use the workgroup barrier; in the persistent
// kernels the four waves of a workgroup run on their own (each spins on its own neighbours), every LDS region a helper
// touches is private to one wave, and LDS operations of one wave execute in order: draining the LDS counter and stopping
// the compiler from moving memory operations across the point is all that is needed.
template <bool WAVE>
__device__ __forceinline__ void spg_node_sync() {
  if constexpr (WAVE) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// 4-term dot product with a FIXED rounding order (explicit fma placement): the per-iteration and the persistent backward
// kernels must produce bit-identical results (tests/test_gpu_ecc_persistent.py), which the compiler's own choice of
// contractions does not guarantee across two different kernels
__device__ __forceinline__ float spg_dot4(const f32x4& w, const f32x4& g) {
  return fmaf(w[0], g[0], w[1] * g[1]) + fmaf(w[2], g[2], w[3] * g[3]);
}

#define SPG_IN_EPS 1e-5f   // nn.InstanceNorm1d(1, eps=1e-5), learning/modules.py:213-214

// in-edge aggregation for node i; result: every lane of the wave holds, for the matrix mode, the 4
// output channels 4*(lane&7)..+3 in a4[]; for the vector mode lanes 0..31 hold channel `lane` in a4[0].
__device__ __forceinline__ void spg_aggregate_node(const SpgGraph& g, const float* __restrict__ W, int matrix,
                                                   const float* __restrict__ hin, long ld, int i, int lane,
                                                   float (&a4)[4]) {
  a4[0] = a4[1] = a4[2] = a4[3] = 0.f;
  const int e0 = g.rowptr[i], e1 = g.rowptr[i + 1];
  if (matrix) {
    const int kb = lane >> 3;
    // 4 edges per batch: all index / filter / state loads of a batch are issued before any of them is consumed
    for (int e = e0; e < e1; e += 4) {
      int sidx[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) sidx[u] = g.src[min(e + u, e1 - 1)];
      f32x4 w[4][4];
      float xk[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const f32x4* We = reinterpret_cast<const f32x4*>(W + (long)min(e + u, e1 - 1) * 1024);
        const float* xj = hin + (long)sidx[u] * ld;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          w[u][q] = We[lane + 64 * q];          // row k = kb + 8q, columns 4*(lane&7)..+3 of W_e[in][out]
          xk[u][q] = xj[kb + 8 * q];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float on = (e + u < e1) ? 1.f : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float xv = xk[u][q] * on;
          a4[0] = fmaf(xv, w[u][q][0], a4[0]);
          a4[1] = fmaf(xv, w[u][q][1], a4[1]);
          a4[2] = fmaf(xv, w[u][q][2], a4[2]);
          a4[3] = fmaf(xv, w[u][q][3], a4[3]);
        }
      }
    }
#pragma unroll
    for (int off = 8; off <= 32; off <<= 1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) a4[c] += __shfl_xor(a4[c], off, 64);
    }
    const float s = g.invdeg[i];
#pragma unroll
    for (int c = 0; c < 4; ++c) a4[c] *= s;
  } else {
    if (lane < 32) {
      float a = 0.f;
      for (int e = e0; e < e1; ++e) a = fmaf(hin[(long)g.src[e] * ld + lane], W[(long)e * 32 + lane], a);
      a4[0] = a * g.invdeg[i];
    }
  }
}

// GRUCellEx forward internals for one node, lane layout:
//   first value  (lanes 0..63): gate pre-activation index `lane`      (0..31 reset chunk, 32..63 update chunk)
//   second value (lanes 0..31): gate pre-activation index 64 + lane   (new-gate chunk)
struct GruFwdState {
  float gin, x;          // input gate and gated input (lanes 0..31)
  float ui1, ui2;        // normalised W_ih x
  float uh1, uh2;        // normalised W_hh h
  float rstd_i, rstd_h;
  float r, z, n;         // gates (lanes 0..31; z was shuffled from lanes 32..63)
};

// Gate rows of the cell's weight matrices, read from a workgroup copy in LDS, rows padded to 33 floats (conflict-free both
// along a row -- the forward dot products -- and along a column -- the backward's W^T products): lane l owns gate rows l
// (first value) and 64 + (l & 31) (GRU) / 64 + l (LSTM) (second value) of W_ih / W_hh and row (l & 31) of the input gate.
#define SPG_WLD 33
struct GruRowsLds {
  const float *ih1, *hh1, *ih2, *hh2, *ig;     // row pointers of this lane
  __device__ __forceinline__ float dot(const float* __restrict__ row, const float* __restrict__ v) const {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(v + 4 * q);   // LDS broadcast read
      a0 = fmaf(row[4 * q + 0], x[0], a0); a1 = fmaf(row[4 * q + 1], x[1], a1);
      a0 = fmaf(row[4 * q + 2], x[2], a0); a1 = fmaf(row[4 * q + 3], x[3], a1);
    }
    return a0 + a1;
  }
  __device__ __forceinline__ float dot_ih1(const float* v) const { return dot(ih1, v); }
  __device__ __forceinline__ float dot_hh1(const float* v) const { return dot(hh1, v); }
  __device__ __forceinline__ float dot_ih2(const float* v) const { return dot(ih2, v); }
  __device__ __forceinline__ float dot_hh2(const float* v) const { return dot(hh2, v); }
  __device__ __forceinline__ float dot_ig(const float* v) const { return dot(ig, v); }
};

// The same rows held in REGISTERS (persistent forward kernel: one wave per SIMD has 512 VGPRs to itself; 160 of them take the
// five rows of this lane, so an iteration's dot products read only the broadcast operand from LDS -- 40 instead of 200 LDS
// reads per lane and iteration).  Same accumulation order as GruRowsLds::dot: the results are bit-identical.
struct GruRowsReg {
  float ih1[32], hh1[32], ih2[32], hh2[32], ig[32];
  __device__ __forceinline__ void load(const GruRowsLds& l) {
#pragma unroll
    for (int k = 0; k < 32; ++k) { ih1[k] = l.ih1[k]; hh1[k] = l.hh1[k]; ih2[k] = l.ih2[k]; hh2[k] = l.hh2[k]; ig[k] = l.ig[k]; }
  }
  static __device__ __forceinline__ float dot(const float (&row)[32], const float* __restrict__ v) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(v + 4 * q);   // LDS broadcast read
      a0 = fmaf(row[4 * q + 0], x[0], a0); a1 = fmaf(row[4 * q + 1], x[1], a1);
      a0 = fmaf(row[4 * q + 2], x[2], a0); a1 = fmaf(row[4 * q + 3], x[3], a1);
    }
    return a0 + a1;
  }
  __device__ __forceinline__ float dot_ih1(const float* v) const { return dot(ih1, v); }
  __device__ __forceinline__ float dot_hh1(const float* v) const { return dot(hh1, v); }
  __device__ __forceinline__ float dot_ih2(const float* v) const { return dot(ih2, v); }
  __device__ __forceinline__ float dot_hh2(const float* v) const { return dot(hh2, v); }
  __device__ __forceinline__ float dot_ig(const float* v) const { return dot(ig, v); }
};

// block-wide: global [GW][32] x2 + [32][32] -> LDS rows of SPG_WLD floats (w_ih | w_hh | w_ig); caller synchronises
template <int GW>
__device__ __forceinline__ void spg_stage_cell_weights(const SpgGruParams& G, float* __restrict__ sw) {
  constexpr int NQ = (2 * GW + 32) * 8;          // float4 pieces
  constexpr int NI = NQ / SPG_THREADS;
  static_assert(NQ % SPG_THREADS == 0, "whole pieces per thread");
  // ALL loads first, then the LDS writes (round 6): as one load-use loop the compiler kept its trips in order -- seven global round
  // trips in a row at the head of the one-launch recurrences (tools/ecc_phase_timing.py: 8 900 cycles)
  f32x4 v[NI];
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const int idx = (int)threadIdx.x + k * SPG_THREADS, row = idx >> 3, q = idx & 7;
    const f32x4* src = row < GW ? reinterpret_cast<const f32x4*>(G.w_ih) + row * 8
                     : (row < 2 * GW ? reinterpret_cast<const f32x4*>(G.w_hh) + (row - GW) * 8
                                     : reinterpret_cast<const f32x4*>(G.ingate ? G.w_ig : G.w_ih) + (row - 2 * GW) * 8);
    v[k] = src[q];
  }
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const int idx = (int)threadIdx.x + k * SPG_THREADS, row = idx >> 3, q = idx & 7;
    float* d = sw + row * SPG_WLD + 4 * q;
    d[0] = v[k][0]; d[1] = v[k][1]; d[2] = v[k][2]; d[3] = v[k][3];
  }
}
template <int CELL>
__device__ __forceinline__ void spg_gru_lds_rows(const float* __restrict__ sw, int lane, GruRowsLds& w) {
  constexpr int GW = CELL == SPG_CELL_LSTM ? 128 : 96;
  const int r1 = lane, r2 = CELL == SPG_CELL_LSTM ? 64 + lane : 64 + (lane & 31);
  w.ih1 = sw + r1 * SPG_WLD; w.ih2 = sw + r2 * SPG_WLD;
  w.hh1 = sw + (GW + r1) * SPG_WLD; w.hh2 = sw + (GW + r2) * SPG_WLD;
  w.ig = sw + (2 * GW + (lane & 31)) * SPG_WLD;
}

// The five bias values a lane adds in the GRU's gates, held in REGISTERS by the one-launch recurrences (loaded once in front of
// the group loop): fetched per iteration they are two dependent cache round trips between "aggregate ready" and "granule
// stored" -- the part of an iteration every neighbour waits for.  The same values enter the same expressions: bit-identical.
// The per-iteration kernels pass none (nullptr) and read the parameter arrays as before.
struct GruLaneBias {
  float ig, ih1, hh1, ih2, hh2;     // b_ig[lane & 31], b_ih[lane], b_hh[lane], b_ih[64 + (lane & 31)], b_hh[64 + (lane & 31)]
  __device__ __forceinline__ void load(const SpgGruParams& G, int lane) {
    ig = G.ingate ? G.b_ig[lane & 31] : 0.f;
    ih1 = G.b_ih[lane]; hh1 = G.b_hh[lane];
    ih2 = G.b_ih[64 + (lane & 31)]; hh2 = G.b_hh[64 + (lane & 31)];
  }
};

template <class Rows, bool WAVE = false>
__device__ __forceinline__ void spg_gru_forward_node(const SpgGruParams& G, const Rows& w, const float* __restrict__ sa,
                                                     const float* __restrict__ sh, float* __restrict__ sx, int lane,
                                                     GruFwdState& st) {
  // No fused multiply-add contraction in here: this function, its two halves below (persistent forward kernel) and the
  // recompute inside the backward kernels must round identically whatever code surrounds them after inlining.
#pragma clang fp contract(off)
  // input gate: x = sigmoid(W_ig h + b_ig) * a      (learning/modules.py:225-226)
  float gin = 1.f, x = 0.f;
  if (lane < 32) {
    if (G.ingate) gin = spg_sigmoid(w.dot_ig(sh) + G.b_ig[lane]);
    x = gin * sa[lane];
    sx[lane] = x;
  }
  st.gin = gin; st.x = x;
  spg_node_sync<WAVE>();
  float gi1 = w.dot_ih1(sx), gh1 = w.dot_hh1(sh);
  float gi2 = 0.f, gh2 = 0.f;
  if (lane < 32) { gi2 = w.dot_ih2(sx); gh2 = w.dot_hh2(sh); }
  st.rstd_i = 1.f; st.rstd_h = 1.f;
  if (G.layernorm) {   // per-row (x - mean)/sqrt(var_biased + eps) over the 96 values (learning/modules.py:218-222)
    const float mi = spg_wave_sum(gi1 + (lane < 32 ? gi2 : 0.f)) * (1.f / 96.f);
    const float mh = spg_wave_sum(gh1 + (lane < 32 ? gh2 : 0.f)) * (1.f / 96.f);
    const float di1 = gi1 - mi, di2 = gi2 - mi, dh1 = gh1 - mh, dh2 = gh2 - mh;
    const float vi = spg_wave_sum(di1 * di1 + (lane < 32 ? di2 * di2 : 0.f)) * (1.f / 96.f);
    const float vh = spg_wave_sum(dh1 * dh1 + (lane < 32 ? dh2 * dh2 : 0.f)) * (1.f / 96.f);
    st.rstd_i = 1.0f / sqrtf(vi + SPG_IN_EPS);
    st.rstd_h = 1.0f / sqrtf(vh + SPG_IN_EPS);
    gi1 = di1 * st.rstd_i; gi2 = di2 * st.rstd_i; gh1 = dh1 * st.rstd_h; gh2 = dh2 * st.rstd_h;
  }
  st.ui1 = gi1; st.ui2 = gi2; st.uh1 = gh1; st.uh2 = gh2;
  // gates (learning/modules.py:242-250): first values are r (lanes 0..31) and z (lanes 32..63)
  const float g1 = spg_sigmoid(((gi1 + G.b_ih[lane]) + gh1) + G.b_hh[lane]);
  st.r = g1;
  st.z = __shfl(g1, (lane & 31) + 32, 64);
  st.n = 0.f;
  if (lane < 32) st.n = tanhf((gi2 + G.b_ih[64 + lane]) + g1 * (gh2 + G.b_hh[64 + lane]));
}


// spg_gru_forward_node in two halves (persistent forward kernel): everything that depends on the node's OWN state only -- the
// input gate, W_hh h and its row normalisation -- is evaluated before the wave starts to wait for its neighbours' states, the
// rest once the aggregate is there.  Same expressions, same order per value as spg_gru_forward_node: bit-identical results
// (tests/test_gpu_ecc_persistent.py compares the two kernels).
template <class Rows>
__device__ __forceinline__ void spg_gru_hidden_part(const SpgGruParams& G, const Rows& w, const float* __restrict__ sh, int lane,
                                                    GruFwdState& st, const GruLaneBias* cb = nullptr) {
#pragma clang fp contract(off)
  float gin = 1.f;
  if (lane < 32 && G.ingate) gin = spg_sigmoid(w.dot_ig(sh) + (cb != nullptr ? cb->ig : G.b_ig[lane]));
  st.gin = gin;
  float gh1 = w.dot_hh1(sh), gh2 = 0.f;
  if (lane < 32) gh2 = w.dot_hh2(sh);
  st.rstd_h = 1.f;
  if (G.layernorm) {
    const float mh = spg_wave_sum(gh1 + (lane < 32 ? gh2 : 0.f)) * (1.f / 96.f);
    const float dh1 = gh1 - mh, dh2 = gh2 - mh;
    const float vh = spg_wave_sum(dh1 * dh1 + (lane < 32 ? dh2 * dh2 : 0.f)) * (1.f / 96.f);
    st.rstd_h = 1.0f / sqrtf(vh + SPG_IN_EPS);
    gh1 = dh1 * st.rstd_h; gh2 = dh2 * st.rstd_h;
  }
  st.uh1 = gh1; st.uh2 = gh2;
}

template <class Rows, bool WAVE>
__device__ __forceinline__ void spg_gru_input_part(const SpgGruParams& G, const Rows& w, const float* __restrict__ sa,
                                                   float* __restrict__ sx, int lane, GruFwdState& st, const GruLaneBias* cb = nullptr) {
#pragma clang fp contract(off)
  float x = 0.f;
  if (lane < 32) {
    x = st.gin * sa[lane];
    sx[lane] = x;
  }
  st.x = x;
  spg_node_sync<WAVE>();
  float gi1 = w.dot_ih1(sx), gi2 = 0.f;
  if (lane < 32) gi2 = w.dot_ih2(sx);
  st.rstd_i = 1.f;
  if (G.layernorm) {
    const float mi = spg_wave_sum(gi1 + (lane < 32 ? gi2 : 0.f)) * (1.f / 96.f);
    const float di1 = gi1 - mi, di2 = gi2 - mi;
    const float vi = spg_wave_sum(di1 * di1 + (lane < 32 ? di2 * di2 : 0.f)) * (1.f / 96.f);
    st.rstd_i = 1.0f / sqrtf(vi + SPG_IN_EPS);
    gi1 = di1 * st.rstd_i; gi2 = di2 * st.rstd_i;
  }
  st.ui1 = gi1; st.ui2 = gi2;
  const float gh1 = st.uh1, gh2 = st.uh2;
  const float g1 = spg_sigmoid(((gi1 + (cb != nullptr ? cb->ih1 : G.b_ih[lane])) + gh1) + (cb != nullptr ? cb->hh1 : G.b_hh[lane]));
  st.r = g1;
  st.z = __shfl(g1, (lane & 31) + 32, 64);
  st.n = 0.f;
  if (lane < 32) st.n = tanhf((gi2 + (cb != nullptr ? cb->ih2 : G.b_ih[64 + lane])) + g1 * (gh2 + (cb != nullptr ? cb->hh2 : G.b_hh[64 + lane])));
}

// forward internals of one (node, iteration) kept for the backward (persistent kernels, training): SPG_PX_SAVE_F values per lane
#define SPG_PX_SAVE_MAGIC 0x53504721u
// three 16-byte stores / loads per lane (1 KiB per wave instruction): `s` points at this lane's first quad, quads 64 apart (the
// backward loads the quads itself, with everything else an iteration reads, and unpacks them behind its gather)
__device__ __forceinline__ void spg_px_save_state(f32x4* __restrict__ s, const GruFwdState& st) {
  const f32x4 a = {st.gin, st.x, st.ui1, st.ui2}, b = {st.uh1, st.uh2, st.rstd_i, st.rstd_h}, c = {st.r, st.z, st.n, 0.f};
  s[0] = a; s[64] = b; s[128] = c;
}
__device__ __forceinline__ void spg_px_unpack_state(const f32x4& a, const f32x4& b, const f32x4& c, GruFwdState& st) {
  st.gin = a[0]; st.x = a[1]; st.ui1 = a[2]; st.ui2 = a[3];
  st.uh1 = b[0]; st.uh2 = b[1]; st.rstd_i = b[2]; st.rstd_h = b[3];
  st.r = c[0]; st.z = c[1]; st.n = c[2];
}

// LSTMCellEx forward internals for one node (learning/modules.py:280-309).  The 128 gate pre-activations
// (chunks i | f | g | o of 32) are two values per lane: index `lane` (i on lanes 0..31, f on 32..63) and index
// 64 + lane (g on lanes 0..31, o on 32..63).  Unlike the GRU, the biases are added BEFORE the row normalisation
// (nnf.linear(input, weight_ih, bias_ih), :297-299).
struct LstmFwdState {
  float gin, x;          // input gate and gated input (lanes 0..31)
  float ui1, ui2;        // normalised W_ih x + b_ih
  float uh1, uh2;        // normalised W_hh h + b_hh
  float rstd_i, rstd_h;
  float i, f, g, o;      // gates, channel = lane (lanes 0..31)
  float c_prev, tc, cy, hy;
};

template <class Rows>
__device__ __forceinline__ void spg_lstm_forward_node(const SpgGruParams& G, const Rows& w, const float* __restrict__ sa,
                                                      const float* __restrict__ sh, float* __restrict__ sx, float c_prev,
                                                      int lane, LstmFwdState& st) {
  float gin = 1.f, x = 0.f;
  if (lane < 32) {
    if (G.ingate) gin = spg_sigmoid(w.dot_ig(sh) + G.b_ig[lane]);      // :285-286, hidden[0]
    x = gin * sa[lane];
    sx[lane] = x;
  }
  st.gin = gin; st.x = x;
  __syncthreads();
  float gi1 = w.dot_ih1(sx) + G.b_ih[lane], gi2 = w.dot_ih2(sx) + G.b_ih[64 + lane];
  float gh1 = w.dot_hh1(sh) + G.b_hh[lane], gh2 = w.dot_hh2(sh) + G.b_hh[64 + lane];
  st.rstd_i = 1.f; st.rstd_h = 1.f;
  if (G.layernorm) {   // InstanceNorm1d over the 128 values of the row, biased variance (:275-279)
    const float mi = spg_wave_sum(gi1 + gi2) * (1.f / 128.f);
    const float mh = spg_wave_sum(gh1 + gh2) * (1.f / 128.f);
    const float di1 = gi1 - mi, di2 = gi2 - mi, dh1 = gh1 - mh, dh2 = gh2 - mh;
    const float vi = spg_wave_sum(di1 * di1 + di2 * di2) * (1.f / 128.f);
    const float vh = spg_wave_sum(dh1 * dh1 + dh2 * dh2) * (1.f / 128.f);
    st.rstd_i = 1.0f / sqrtf(vi + SPG_IN_EPS);
    st.rstd_h = 1.0f / sqrtf(vh + SPG_IN_EPS);
    gi1 = di1 * st.rstd_i; gi2 = di2 * st.rstd_i; gh1 = dh1 * st.rstd_h; gh2 = dh2 * st.rstd_h;
  }
  st.ui1 = gi1; st.ui2 = gi2; st.uh1 = gh1; st.uh2 = gh2;
  const float p1 = gi1 + gh1, p2 = gi2 + gh2;
  const float v1 = spg_sigmoid(p1);                         // i (lanes 0..31) / f (lanes 32..63)
  const float v2 = lane < 32 ? tanhf(p2) : spg_sigmoid(p2); // g (lanes 0..31) / o (lanes 32..63)
  st.i = v1; st.g = v2;
  st.f = __shfl(v1, (lane & 31) + 32, 64);
  st.o = __shfl(v2, (lane & 31) + 32, 64);
  st.c_prev = c_prev;
  st.cy = st.f * c_prev + st.i * st.g;                      // :306
  st.tc = tanhf(st.cy);
  st.hy = st.o * st.tc;                                     // :307
}

// ---------------------------------------------------------------------------------------------
// forward step
// ---------------------------------------------------------------------------------------------
// The cell's weight matrices are staged once per workgroup in LDS (rows padded to SPG_WLD floats) and every lane reads its
// gate rows from there: 103-168 VGPRs, 3-4 waves per SIMD.  (Register-resident rows -- 264 VGPRs, one wave per SIMD -- were
// measured slower at every graph size: 1 scene 1.83 -> 1.79 ms/step, 8 scenes 811k -> 887k superpoints/s.)
template <int CELL>
__global__ __launch_bounds__(256, 3) void spg_ecc_step_fwd_kernel(const SpgEccStepFwd p) {
  constexpr int GW = CELL == SPG_CELL_LSTM ? 128 : 96;
  __shared__ __attribute__((aligned(16))) float lds[4][3][32];
  __shared__ float sw[(2 * GW + 32) * SPG_WLD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  const bool active = i < p.g.N;
  GruRowsLds wr;
  if (p.do_gru) spg_stage_cell_weights<GW>(p.gru, sw);          // visible after the barrier behind the aggregation
  spg_gru_lds_rows<CELL>(sw, lane, wr);
  float* sa = lds[wave][0];
  float* sh = lds[wave][1];
  float* sx = lds[wave][2];
  if (active) {
    if (p.agg_in != nullptr) {
      if (lane < 32) sa[lane] = p.agg_in[(long)i * p.ldagg + lane];
    } else {
      float a4[4];
      spg_aggregate_node(p.g, p.W, p.matrix, p.hin, p.ld, i, lane, a4);
      if (p.matrix) {
        if (lane < 8) {
          sa[4 * lane + 0] = a4[0]; sa[4 * lane + 1] = a4[1]; sa[4 * lane + 2] = a4[2]; sa[4 * lane + 3] = a4[3];
        }
      } else if (lane < 32) {
        sa[lane] = a4[0];
      }
    }
    if (lane < 32 && p.do_gru) sh[lane] = p.hin[(long)i * p.ld + lane];
  } else if (lane < 32) {
    sa[lane] = 0.f; sh[lane] = 0.f;
  }
  __syncthreads();
  if (active && p.agg_save != nullptr && lane < 32) p.agg_save[(long)i * p.ldagg + lane] = sa[lane];
  if (!p.do_gru) return;
  if constexpr (CELL == SPG_CELL_GRU) {
    GruFwdState st;
    spg_gru_forward_node(p.gru, wr, sa, sh, sx, lane, st);
    if (active && lane < 32) {
      const float h = sh[lane];
      p.hout[(long)i * p.ld + lane] = st.n + st.z * (h - st.n);   // hy = newgate + inputgate*(hidden - newgate)
    }
  } else {
    LstmFwdState st;
    const float c = (active && lane < 32 && p.cin != nullptr) ? p.cin[(long)i * p.ld + lane] : 0.f;
    spg_lstm_forward_node(p.gru, wr, sa, sh, sx, c, lane, st);
    if (active && lane < 32) {
      p.hout[(long)i * p.ld + lane] = st.hy;
      p.cout[(long)i * p.ld + lane] = st.cy;
    }
  }
}

int spg_launch_ecc_step_fwd(const SpgEccStepFwd& p, hipStream_t stream) {
  const dim3 grid(spg_cdiv(p.g.N, 4));
  if (p.cell == SPG_CELL_LSTM) hipLaunchKernelGGL(spg_ecc_step_fwd_kernel<SPG_CELL_LSTM>, grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(spg_ecc_step_fwd_kernel<SPG_CELL_GRU>, grid, dim3(256), 0, stream, p);
  SPG_LAUNCH_CHECK();
  return 0;
}

// GRUCellEx backward for one node (one wavefront): recompute of the forward from (aggregate sa[0..31], state sh[0..31]),
// gate gradients stored for the deferred weight-gradient GEMMs, returns the gradient wrt the hidden state (direct path,
// dh_acc) and wrt the aggregate (da), lanes 0..31.  sa / sh are GW = 96 floats each (re-used for dgi / dgh), sx and sd 32;
// sw is the workgroup's padded copy of the cell weights.  DEPTH / DEPTH_IG: gate rows per batch of LDS reads in the W^T / input-gate
// products -- 2 (1) registers per row plus the operand quads, so as deep as the instantiation's registers allow (24 / 32 with one
// workgroup per CU, 16 everywhere else -- 4 made the iteration-major backward 2 % slower: profiles/ecc_cell_lds_{isa,ab}.txt).
struct SpgGruBwdOut { float *dgi, *dgh, *dui, *duh, *dpre, *xg; long ld96, ld32; };

template <bool WAVE, int DEPTH = 16, int DEPTH_IG = DEPTH>
__device__ __forceinline__ void spg_gru_backward_node(const SpgGruParams& G, const float* __restrict__ sw, float* sa, float* sh,
                                                      float* sx, float* sd, int lane, bool active, long j, float dH,
                                                      const SpgGruBwdOut& o, float& dh_acc, float& da,
                                                      const GruFwdState* saved = nullptr, bool use_saved = true,
                                                      const GruLaneBias* cb = nullptr) {
  constexpr int GW = 96;
  const float* sw_ih = sw;
  const float* sw_hh = sw_ih + GW * SPG_WLD;
  const float* sw_ig = sw_hh + GW * SPG_WLD;
  {
    GruFwdState st;
    if (saved != nullptr && use_saved) {      // the forward kernel kept its internals (persistent kernels): nothing to recompute
      st = *saved;
    } else {
      GruRowsLds wr;
      spg_gru_lds_rows<SPG_CELL_GRU>(sw, lane, wr);
      spg_gru_forward_node<GruRowsLds, WAVE>(G, wr, sa, sh, sx, lane, st);
    }
    const float a_in = lane < 32 ? sa[lane] : 0.f;
    const float h_in = lane < 32 ? sh[lane] : 0.f;
    // gate backward on lanes 0..31 (channel = lane)
    float dr_pre = 0.f, dz_pre = 0.f, dn_pre = 0.f;
    dh_acc = 0.f;
    if (lane < 32) {
      const float dn = dH * (1.f - st.z);
      const float dzg = dH * (h_in - st.n);
      dh_acc = dH * st.z;
      dn_pre = dn * (1.f - st.n * st.n);
      const float dr = dn_pre * (st.uh2 + (cb != nullptr ? cb->hh2 : G.b_hh[64 + lane]));
      dz_pre = dzg * st.z * (1.f - st.z);
      dr_pre = dr * st.r * (1.f - st.r);
    }
    // gradients wrt the normalised pre-activations, in the first/second-value lane layout
    const float zsh = __shfl(dz_pre, lane & 31, 64);
    float dui1 = lane < 32 ? dr_pre : zsh;        // index lane
    float dui2 = lane < 32 ? dn_pre : 0.f;        // index 64 + lane
    float duh1 = dui1;
    float duh2 = lane < 32 ? dn_pre * st.r : 0.f;
    if (active) {
      o.dui[(long)j * o.ld96 + lane] = dui1;
      o.duh[(long)j * o.ld96 + lane] = duh1;
      if (lane < 32) {
        o.dui[(long)j * o.ld96 + 64 + lane] = dui2;
        o.duh[(long)j * o.ld96 + 64 + lane] = duh2;
      }
    }
    // through the row normalisation: dg = rstd * (du - mean(du) - u * mean(du*u))
    float dgi1 = dui1, dgi2 = dui2, dgh1 = duh1, dgh2 = duh2;
    if (G.layernorm) {
      const float m1i = spg_wave_sum(dui1 + dui2) * (1.f / 96.f);
      const float m2i = spg_wave_sum(dui1 * st.ui1 + dui2 * st.ui2) * (1.f / 96.f);
      const float m1h = spg_wave_sum(duh1 + duh2) * (1.f / 96.f);
      const float m2h = spg_wave_sum(duh1 * st.uh1 + duh2 * st.uh2) * (1.f / 96.f);
      dgi1 = st.rstd_i * (dui1 - m1i - st.ui1 * m2i);
      dgi2 = st.rstd_i * (dui2 - m1i - st.ui2 * m2i);
      dgh1 = st.rstd_h * (duh1 - m1h - st.uh1 * m2h);
      dgh2 = st.rstd_h * (duh2 - m1h - st.uh2 * m2h);
    }
    spg_node_sync<WAVE>();   // sa/sh (as inputs) are no longer needed by any lane of this wave
    sa[lane] = dgi1;
    sh[lane] = dgh1;
    if (lane < 32) { sa[64 + lane] = dgi2; sh[64 + lane] = dgh2; }
    if (active) {
      o.dgi[(long)j * o.ld96 + lane] = dgi1;
      o.dgh[(long)j * o.ld96 + lane] = dgh1;
      if (lane < 32) {
        o.dgi[(long)j * o.ld96 + 64 + lane] = dgi2;
        o.dgh[(long)j * o.ld96 + 64 + lane] = dgh2;
      }
    }
    spg_node_sync<WAVE>();
    // W^T products dx[c] = sum_o W_ih[o][c] dgi[o], dh[c] += sum_o W_hh[o][c] dgh[o]: the 96 gate rows are split over the two
    // half-waves (48 each) and over two accumulators, so the dependent fma chain is 24 long instead of 96; the halves meet
    // through one cross-row shuffle
    //
    // The LDS reads of a product are issued in BATCHES of DEPTH gate rows (weights: one value per row and matrix, by column;
    // operands: contiguous, 128-bit broadcasts), all of a batch in front of its multiply-adds, and the loop counter is the same
    // for every lane (the half-wave's first row is in the addresses).  Written as one load-use loop from a per-lane first row,
    // the compiler built a divergent loop plus a remainder loop and waited for every pair of weights where it was used: 64
    // dependent LDS round trips per node and iteration for 128 multiply-adds per lane, with one wavefront per SIMD and nothing
    // to switch to.  The empty asm statements behind a batch keep the reads from sinking back to their uses.  Every
    // multiply-add, its operands and the order within each of the four accumulator chains are unchanged: bit-identical.
    float dx;
    {
      static_assert(DEPTH % 4 == 0 && 48 % DEPTH == 0, "whole batches of operand quads per half-wave");
      const int c = lane & 31, q0 = 48 * (lane >> 5);
      const float* wi = sw_ih + q0 * SPG_WLD + c;
      const float* wh = sw_hh + q0 * SPG_WLD + c;
      const f32x4* pa = reinterpret_cast<const f32x4*>(sa + q0);
      const f32x4* ph = reinterpret_cast<const f32x4*>(sh + q0);
      float x0 = 0.f, x1 = 0.f, h0 = 0.f, h1 = 0.f;
#pragma unroll
      for (int t0 = 0; t0 < 48; t0 += DEPTH) {
        float wiv[DEPTH], whv[DEPTH];
        f32x4 av[DEPTH / 4], hv[DEPTH / 4];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) { wiv[k] = wi[(t0 + k) * SPG_WLD]; whv[k] = wh[(t0 + k) * SPG_WLD]; }
#pragma unroll
        for (int k = 0; k < DEPTH / 4; ++k) { av[k] = pa[t0 / 4 + k]; hv[k] = ph[t0 / 4 + k]; }
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) { asm volatile("" : "+v"(wiv[k])); asm volatile("" : "+v"(whv[k])); }
#pragma unroll
        for (int k = 0; k < DEPTH / 4; ++k) { asm volatile("" : "+v"(av[k])); asm volatile("" : "+v"(hv[k])); }
#pragma unroll
        for (int k = 0; k < DEPTH; k += 2) {
          x0 = fmaf(wiv[k], av[k >> 2][k & 3], x0);
          x1 = fmaf(wiv[k + 1], av[k >> 2][(k & 3) + 1], x1);
          h0 = fmaf(whv[k], hv[k >> 2][k & 3], h0);
          h1 = fmaf(whv[k + 1], hv[k >> 2][(k & 3) + 1], h1);
        }
      }
      float xs = x0 + x1, hs_ = h0 + h1;
      xs += __shfl_xor(xs, 32, 64);
      hs_ += __shfl_xor(hs_, 32, 64);
      dx = lane < 32 ? xs : 0.f;
      if (lane < 32) dh_acc += hs_;
    }
    da = dx;
    float dpre = 0.f;
    if (G.ingate) {
      da = dx * st.gin;
      dpre = dx * a_in * st.gin * (1.f - st.gin);
      if (lane < 32) sd[lane] = dpre;
    }
    spg_node_sync<WAVE>();
    if (G.ingate && lane < 32) {
      float g0 = 0.f, g1 = 0.f;
      constexpr int DG = DEPTH_IG;      // (the same batching: DG rows of W_ig by column, the operand as 128-bit broadcasts)
      static_assert(DG % 4 == 0 && 32 % DG == 0, "whole batches of operand quads");
      const float* wg = sw_ig + lane;
      const f32x4* pd = reinterpret_cast<const f32x4*>(sd);
#pragma unroll
      for (int t0 = 0; t0 < 32; t0 += DG) {
        float wgv[DG];
        f32x4 dv[DG / 4];
#pragma unroll
        for (int k = 0; k < DG; ++k) wgv[k] = wg[(t0 + k) * SPG_WLD];
#pragma unroll
        for (int k = 0; k < DG / 4; ++k) dv[k] = pd[t0 / 4 + k];
#pragma unroll
        for (int k = 0; k < DG; ++k) asm volatile("" : "+v"(wgv[k]));
#pragma unroll
        for (int k = 0; k < DG / 4; ++k) asm volatile("" : "+v"(dv[k]));
#pragma unroll
        for (int k = 0; k < DG; k += 2) {
          g0 = fmaf(wgv[k], dv[k >> 2][k & 3], g0);
          g1 = fmaf(wgv[k + 1], dv[k >> 2][(k & 3) + 1], g1);
        }
      }
      dh_acc += g0 + g1;
    }
    if (active && lane < 32) {
      o.dpre[(long)j * o.ld32 + lane] = dpre;
      o.xg[(long)j * o.ld32 + lane] = st.x;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// backward step
// ---------------------------------------------------------------------------------------------
template <int CELL>
__global__ __launch_bounds__(256, 3) void spg_ecc_step_bwd_kernel(const SpgEccStepBwd p) {
  constexpr int GW = CELL == SPG_CELL_LSTM ? 128 : 96;
  __shared__ __attribute__((aligned(16))) float lds[4][5][GW];
  // the backward needs COLUMNS of the weight matrices (dx[c] = sum_o W[o][c] dg[o]): the block stages them in LDS once
  // (loads issued here, in flight during the reverse gather) instead of 2*GW+32 global loads per lane
  constexpr int WQ = (2 * GW * 32 + 1024) / 4;                   // float4 pieces: w_ih | w_hh | w_ig
  __shared__ float sw[(2 * GW + 32) * SPG_WLD];                   // rows padded to SPG_WLD: conflict-free along rows and columns
  constexpr int WPT = (WQ + SPG_THREADS - 1) / SPG_THREADS;
  f32x4 wreg[WPT];
  if (!p.final_only) {
#pragma unroll
    for (int u = 0; u < WPT; ++u) {
      const int idx = threadIdx.x + SPG_THREADS * u;
      const int ii = idx < WQ ? idx : 0;
      const f32x4* src = ii < GW * 8 ? reinterpret_cast<const f32x4*>(p.gru.w_ih) + ii
                       : (ii < 2 * GW * 8 ? reinterpret_cast<const f32x4*>(p.gru.w_hh) + (ii - GW * 8)
                                          : reinterpret_cast<const f32x4*>(p.gru.ingate ? p.gru.w_ig : p.gru.w_ih) + (ii - 2 * GW * 8));
      wreg[u] = *src;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * 4 + wave;
  const bool active = j < p.g.N;
  float* sa = lds[wave][0];        // [32] aggregate   | later dgi [96]
  float* sh = lds[wave][1];        // [32] hidden      | later dgh [96]
  float* sx = lds[wave][2];        // [32] gated input
  float* sd = lds[wave][3];        // [32] dH          | later dpre [32]
  // ---- phase 1: total gradient wrt the state produced by this iteration ----
  float dH = 0.f;   // lanes 0..31
  if (active) {
    if (lane < 32) {
      if (p.dcat != nullptr) dH += p.dcat[(long)j * p.ldc + lane];
      if (p.use_dhdir) dH += p.dhdir[(long)j * 32 + lane];
    }
    if (p.Gnext != nullptr) {
      const int b = p.g.rev_rowptr[j], e_ = p.g.rev_rowptr[j + 1];
      if (p.matrix) {
        float pq[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = b; t < e_; t += 4) {      // 4 out-edges per batch, loads first
          int eid[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) eid[u] = p.g.rev_eid[min(t + u, e_ - 1)];
          int did[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) did[u] = p.g.dst[eid[u]];
          f32x4 w[4][4], g4[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            g4[u] = *reinterpret_cast<const f32x4*>(p.Gnext + (long)did[u] * p.ldg + 4 * (lane & 7));
            const f32x4* We = reinterpret_cast<const f32x4*>(p.W + (long)eid[u] * 1024);
#pragma unroll
            for (int q = 0; q < 4; ++q) w[u][q] = We[lane + 64 * q];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float on = (t + u < e_) ? 1.f : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q)
              pq[q] += on * spg_dot4(w[u][q], g4[u]);
          }
        }
#pragma unroll
        for (int off = 1; off <= 4; off <<= 1) {
#pragma unroll
          for (int q = 0; q < 4; ++q) pq[q] += __shfl_xor(pq[q], off, 64);
        }
        if ((lane & 7) == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) sd[(lane >> 3) + 8 * q] = pq[q];   // input channel k = lane/8 + 8q
        }
      } else if (lane < 32) {
        float s = 0.f;
        for (int t = b; t < e_; ++t) {
          const int e = p.g.rev_eid[t];
          s = fmaf(p.W[(long)e * 32 + lane], p.Gnext[(long)p.g.dst[e] * p.ldg + lane], s);
        }
        sd[lane] = s;
      }
    } else if (lane < 32) {
      sd[lane] = 0.f;
    }
  } else if (lane < 32) {
    sd[lane] = 0.f;
  }
  __syncthreads();
  if (lane < 32) dH += sd[lane];
  if (p.final_only) {
    if (active && lane < 32) p.gx[(long)j * 32 + lane] = dH;
    return;
  }
  // ---- phase 2: recompute the GRU forward of this iteration, then its backward ----
  if (lane < 32) {
    sa[lane] = active ? p.agg[(long)j * p.ldagg + lane] : 0.f;
    sh[lane] = active ? p.hin[(long)j * p.ld + lane] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < WPT; ++u) {
    const int idx = threadIdx.x + SPG_THREADS * u;
    if (idx < WQ) {
      float* d = sw + (idx >> 3) * SPG_WLD + 4 * (idx & 7);
      d[0] = wreg[u][0]; d[1] = wreg[u][1]; d[2] = wreg[u][2]; d[3] = wreg[u][3];
    }
  }
  const float* sw_ih = sw;
  const float* sw_hh = sw_ih + GW * SPG_WLD;
  const float* sw_ig = sw_hh + GW * SPG_WLD;
  __syncthreads();
  const SpgGruParams& G = p.gru;
  if constexpr (CELL == SPG_CELL_LSTM) {
    // ---- LSTMCellEx backward (learning/modules.py:280-309) ----
    LstmFwdState st;
    {
      const float c = (active && lane < 32 && p.cin != nullptr) ? p.cin[(long)j * p.ld + lane] : 0.f;
      GruRowsLds wr;
      spg_gru_lds_rows<SPG_CELL_LSTM>(sw, lane, wr);
      spg_lstm_forward_node(G, wr, sa, sh, sx, c, lane, st);
    }
    const float a_in = lane < 32 ? sa[lane] : 0.f;
    // gate backward on lanes 0..31 (channel = lane):  hy = o tanh(cy),  cy = f c + i g
    float di_pre = 0.f, df_pre = 0.f, dg_pre = 0.f, do_pre = 0.f, dc_prev = 0.f;
    if (lane < 32) {
      float dC = dH * st.o * (1.f - st.tc * st.tc);
      if (p.use_dcdir && active) dC += p.dcdir[(long)j * 32 + lane];
      do_pre = dH * st.tc * st.o * (1.f - st.o);
      di_pre = dC * st.g * st.i * (1.f - st.i);
      df_pre = dC * st.c_prev * st.f * (1.f - st.f);
      dg_pre = dC * st.i * (1.f - st.g * st.g);
      dc_prev = dC * st.f;
    }
    // gradient wrt the sum of the two normalised pre-activations, in the two-values-per-lane layout
    const float fsh = __shfl(df_pre, lane & 31, 64), osh = __shfl(do_pre, lane & 31, 64);
    const float du1 = lane < 32 ? di_pre : fsh;      // index lane
    const float du2 = lane < 32 ? dg_pre : osh;      // index 64 + lane
    float dgi1 = du1, dgi2 = du2, dgh1 = du1, dgh2 = du2;
    if (G.layernorm) {
      const float m1 = spg_wave_sum(du1 + du2) * (1.f / 128.f);
      const float m2i = spg_wave_sum(du1 * st.ui1 + du2 * st.ui2) * (1.f / 128.f);
      const float m2h = spg_wave_sum(du1 * st.uh1 + du2 * st.uh2) * (1.f / 128.f);
      dgi1 = st.rstd_i * (du1 - m1 - st.ui1 * m2i);
      dgi2 = st.rstd_i * (du2 - m1 - st.ui2 * m2i);
      dgh1 = st.rstd_h * (du1 - m1 - st.uh1 * m2h);
      dgh2 = st.rstd_h * (du2 - m1 - st.uh2 * m2h);
    }
    __syncthreads();   // sa/sh (as inputs) are no longer needed by any lane of this wave
    sa[lane] = dgi1; sa[64 + lane] = dgi2;
    sh[lane] = dgh1; sh[64 + lane] = dgh2;
    if (active) {
      p.dgi[(long)j * p.ld96 + lane] = dgi1; p.dgi[(long)j * p.ld96 + 64 + lane] = dgi2;
      p.dgh[(long)j * p.ld96 + lane] = dgh1; p.dgh[(long)j * p.ld96 + 64 + lane] = dgh2;
    }
    __syncthreads();
    float dx = 0.f, dh_acc = 0.f;
    if (lane < 32) {
#pragma unroll 8
      for (int o = 0; o < 128; ++o) {
        dx = fmaf(sw_ih[o * SPG_WLD + lane], sa[o], dx);
        dh_acc = fmaf(sw_hh[o * SPG_WLD + lane], sh[o], dh_acc);
      }
    }
    float da = dx, dpre = 0.f;
    if (G.ingate) {
      da = dx * st.gin;
      dpre = dx * a_in * st.gin * (1.f - st.gin);
      if (lane < 32) sd[lane] = dpre;
    }
    __syncthreads();
    if (G.ingate && lane < 32) {
#pragma unroll 8
      for (int o = 0; o < 32; ++o) dh_acc = fmaf(sw_ig[o * SPG_WLD + lane], sd[o], dh_acc);
    }
    if (active && lane < 32) {
      p.dpre[(long)j * p.ld32 + lane] = dpre;
      p.xg[(long)j * p.ld32 + lane] = st.x;
      p.dhdir[(long)j * 32 + lane] = dh_acc;
      p.dcdir[(long)j * 32 + lane] = dc_prev;
      p.Gcur[(long)j * p.ldg + lane] = p.g.invdeg != nullptr ? da * p.g.invdeg[j] : da;
    }
  } else {
    SpgGruBwdOut o;
    o.dgi = p.dgi; o.dgh = p.dgh; o.dui = p.dui; o.duh = p.duh; o.dpre = p.dpre; o.xg = p.xg; o.ld96 = p.ld96; o.ld32 = p.ld32;
    float dh_acc, da;
    spg_gru_backward_node<false>(G, sw, sa, sh, sx, sd, lane, active, j, dH, o, dh_acc, da);
    if (active && lane < 32) {
      p.dhdir[(long)j * 32 + lane] = dh_acc;
      p.Gcur[(long)j * p.ldg + lane] = p.g.invdeg != nullptr ? da * p.g.invdeg[j] : da;
    }
  }
}

int spg_launch_ecc_step_bwd(const SpgEccStepBwd& p, hipStream_t stream) {
  const dim3 grid(spg_cdiv(p.g.N, 4));
  if (p.cell == SPG_CELL_LSTM) hipLaunchKernelGGL(spg_ecc_step_bwd_kernel<SPG_CELL_LSTM>, grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(spg_ecc_step_bwd_kernel<SPG_CELL_GRU>, grid, dim3(256), 0, stream, p);
  SPG_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// per-edge filter gradient, summed over the R iterations in registers (written once)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spg_ecc_edge_wgrad_kernel(const SpgEdgeWgrad p) {
  spg_ecc_edge_wgrad_body(p, (int)blockIdx.x);
}

int spg_launch_ecc_edge_wgrad(const SpgGraph& g, int matrix, const float* states, long lds, const float* G, long ldg,
                              int R, float* dW, hipStream_t stream) {
  if (g.E == 0) return 0;
  SpgEdgeWgrad p;
  p.g = g; p.matrix = matrix; p.states = states; p.lds = lds; p.G = G; p.ldg = ldg; p.R = R; p.dW = dW;
  if (spg_group_add_edge_wgrad(p, stream)) return 0;      // inside a grouped launch (spg_gemm.h)
  hipLaunchKernelGGL(spg_ecc_edge_wgrad_kernel, dim3(spg_cdiv(g.E, 4)), dim3(256), 0, stream, p);
  SPG_LAUNCH_CHECK();
  return 0;
}

__global__ void spg_copy2d_kernel(const float* __restrict__ src, long lds_, float* __restrict__ dst, long ldd, long rows,
                                  int cols) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols) return;
  const long r = i / cols;
  const int c = (int)(i - r * cols);
  dst[r * ldd + c] = src[r * lds_ + c];
}

int spg_launch_copy2d(const float* src, long lds, float* dst, long ldd, long rows, int cols, hipStream_t stream) {
  const long n = rows * cols;
  if (n == 0) return 0;
  hipLaunchKernelGGL(spg_copy2d_kernel, dim3(spg_cdiv(n, 256)), dim3(256), 0, stream, src, lds, dst, ldd, rows, cols);
  SPG_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Persistent RNN-ECC: all R iterations of the recurrence in ONE launch, synchronised by DATAFLOW
// ---------------------------------------------------------------------------------------------
// reference: RNNGraphConvModule.forward, learning/modules.py:171-181 (the loop over nrepeats); GraphConvFunction
// forward / backward, learning/ecc/GraphConvModule.py:44-152; GRUCellEx, learning/modules.py:224-251.
//
// Node i at iteration r+1 needs nothing but the iteration-r states of its <= deg(i) in-neighbours -- no grid-wide barrier.
// One wavefront owns one node for the whole recurrence (N <= 1024 nodes: <= 256 workgroups of 4 waves, all co-resident),
// publishes every new state as 32 eight-byte {tag, value} granules with write-through (sc1) stores and, for the next
// iteration, sweeps the granules of its sources until every tag carries the expected epoch (cdna guide, guideline 16,
// form R2: the data is the flag -- no fences, no separate flag round trip; measured price of a hop ~1 us against ~9 us for a
// per-iteration launch of this latency-bound step).  What stays on chip for all iterations: the node's in-edge (forward) or
// out-edge (backward) filters in registers (up to SPG_PX_KMAX edges x 4 KiB per wave; further edges are re-read through L2),
// its edge list, the cell's weights in LDS, its own state.  The plain outputs the later kernels need (states, aggregates,
// gate gradients) are written with ordinary stores; only the exchanged vectors travel as granules.
//
// The exchange buffer is the second piece of device memory the library owns (per device, SPG_PX_MAX_GROUPS x SPG_PX_MAX_ITERS x SPG_PX_MAX_NODES x 256 B = 64 MiB + a control block; allocated on first use): epochs are
// drawn from a device-side counter that the last workgroup of a launch advances, so a tag is never reused -- neither across
// launches nor under hipGraph replay -- and the buffer needs no clearing.  One persistent launch is in flight per device at a
// time (launches of one stream serialise; a second stream falls back to the per-iteration kernels).  Spins are bounded: a
// wave that waits longer than SPG_PX_SPIN_LIMIT sweeps raises the error word of the control block (spg_ecc_persistent_errors)
// and carries on, so a logic error can never hang the GPU.
#define SPG_PX_KMAX1 12        // edges per node whose filters stay in registers (16 VGPRs each in matrix mode), one workgroup per CU
#define SPG_PX_KMAX2 6         // ... with two workgroups per CU (256 VGPRs per wave), forward
#define SPG_PX_KMAX2B 2        // ... backward
#define SPG_PX_CH 32           // edges gathered per pass (wave-private LDS staging)
#define SPG_PX_SPIN_LIMIT 400000
#define SPG_PX_SPIN_FORCED 0xffffffffu   // spg_tune key 20 = -1: every wait reports a time-out at once (tests; the data may or may not be stale)

typedef __attribute__((address_space(1))) unsigned long long spg_gu64;
typedef __attribute__((address_space(1))) unsigned spg_gu32;

__device__ __forceinline__ void spg_px_store_granule(unsigned long long* g, unsigned tag, float v) {
  __hip_atomic_store((spg_gu64*)g, ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// One wave gathers the 32-float vectors of `n` (<= SPG_PX_CH) peers into hs[u][0..31]: lanes 0..31 take even, lanes 32..63 odd
// list positions.  Plain form (rows of a finished matrix, leading dimension ld) or granule form (tags must equal `tag`;
// swept until they do).  ids: wave-private LDS list of the peers' node indices.
// rowidx (optional): row i of X is X[rowidx[i]], a ZERO row where rowidx[i] < 0 -- the embedding scatter of CloudEmbedder
// (learning/pointnet.py:177-179) read in place instead of through a materialised descriptor matrix
__device__ __forceinline__ void spg_px_gather_plain(const float* __restrict__ X, long ld, const int* ids, int n, int lane, float* hs,
                                                    const int64_t* __restrict__ rowidx = nullptr) {
  const int half = lane >> 5, c = lane & 31;
  for (int p = 0; p < n; p += 8) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int u = p + 2 * k + half;
      long row = ids[u < n ? u : 0];
      if (rowidx != nullptr) row = rowidx[row];
      v[k] = row >= 0 ? X[row * ld + c] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int u = p + 2 * k + half;
      if (u < n) hs[u * 32 + c] = v[k];
    }
  }
}

// PER entries per half wave and sweep (2 * PER peers per round): a node with more than 8 peers would otherwise need a second
// round -- a second hop latency on the path of the nodes that gate their neighbourhood
template <int PER>
__device__ __forceinline__ void spg_px_gather_granules_t(const unsigned long long* __restrict__ gran, unsigned tag, const int* ids,
                                                         int n, int lane, float* hs, unsigned* ctl, unsigned limit) {
  const int half = lane >> 5, c = lane & 31;
  for (int p = 0; p < n; p += 2 * PER) {
    for (unsigned spins = 0;; ++spins) {
      unsigned long long x[PER];
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int u = p + 2 * k + half;
        x[k] = __hip_atomic_load((spg_gu64*)(gran + (long)ids[u < n ? u : 0] * 32 + c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      bool ok = true;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int u = p + 2 * k + half;
        if (u < n) ok = ok && (unsigned)(x[k] >> 32) == tag;
      }
      const bool done = __all(ok);
      const bool forced = limit == SPG_PX_SPIN_FORCED;       // (uniform; the tests' deterministic time-out)
      if (done || forced || spins > limit) {
        if ((!done || forced) && lane == 0) atomicAdd(ctl + 2, 1u);   // never hang: flag the error and go on with what is there
#pragma unroll
        for (int k = 0; k < PER; ++k) {
          const int u = p + 2 * k + half;
          if (u < n) hs[u * 32 + c] = __uint_as_float((unsigned)x[k]);
        }
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
}

__device__ __forceinline__ void spg_px_gather_granules(const unsigned long long* __restrict__ gran, unsigned tag, const int* ids,
                                                       int n, int lane, float* hs, unsigned* ctl, unsigned limit) {
  if (n <= 8) spg_px_gather_granules_t<4>(gran, tag, ids, n, lane, hs, ctl, limit);
  else spg_px_gather_granules_t<8>(gran, tag, ids, n, lane, hs, ctl, limit);
}

// the bound of the waits: the built-in one, or the (smaller) one of spg_tune key 20 in ctl[4] -- the fail-safe tests force a
// time-out with it; read once per wave (a scalar load)
__device__ __forceinline__ unsigned spg_px_spin_limit(const unsigned* ctl) {
  const unsigned v = __hip_atomic_load((spg_gu32*)(ctl + 4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (v == SPG_PX_SPIN_FORCED) return v;
  return v != 0u && v < (unsigned)SPG_PX_SPIN_LIMIT ? v : (unsigned)SPG_PX_SPIN_LIMIT;
}

// the last workgroup to finish advances the epoch base past every tag this launch used and re-arms the counter
// (counted when wave 0 of a workgroup is through -- wave 0 always owns a node; what matters is that every workgroup has
// read the base before it moves, and the last arrival implies that all have started)
__device__ __forceinline__ void spg_px_finish(unsigned* ctl, unsigned base, unsigned used) {
  if (threadIdx.x == 0) {
    const unsigned prev = __hip_atomic_fetch_add((spg_gu32*)(ctl + 1), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {
      __hip_atomic_store((spg_gu32*)(ctl + 1), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store((spg_gu32*)ctl, base + used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__device__ __forceinline__ int spg_opaque_lane_zero() { int z = 0; asm volatile("" : "+v"(z)); return z; }
// the cell's gate rows of a lane: a register copy (one workgroup per CU) or the LDS row pointers themselves
template <bool REG> struct SpgPxRows { typedef GruRowsReg type; };
template <> struct SpgPxRows<false> { typedef GruRowsLds type; };
__device__ __forceinline__ void spg_px_rows_init(GruRowsReg& w, const GruRowsLds& l) { w.load(l); }
__device__ __forceinline__ void spg_px_rows_init(GruRowsLds& w, const GruRowsLds& l) { w = l; }

// ---- the head behind the recurrence (SpgEccHead, spg_ecc.h): classifier + weighted cross entropy per node, in the owning wave ----
// The four 64-lane float64 butterflies of a thread, step by step SIDE BY SIDE: the four exchanges of a step are independent and share
// one LDS-crossbar round trip (as four loops in a row they were 24 dependent round trips of two ds_bpermute each at the forward's
// entry); each sum keeps its own pairwise order, so its bits.
__device__ __forceinline__ void spg_wave_sum4_f64(double (&acc)[4]) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    double o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = __shfl_xor(acc[q], off, 64);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] += o[q];
  }
}
// Sum over ALL rows of the labelled rows' class weights -- the normaliser of the mean reduction -- by the 256 threads of a
// workgroup, with the summation order of ce_fwd_kernel (spg_loss.hip): 1024 virtual threads striding the rows, a 64-lane butterfly
// per virtual wave, the 16 wave sums added in order.  Thread p plays the virtual threads p, p + 256, p + 512, p + 768 (virtual
// wave (p >> 6) + 4q = its own wave's butterfly).  part: [16] doubles in LDS; every caller adds them up itself after the next
// workgroup barrier (spg_px_head_wsum_finish) -- the same value in every workgroup and every launch.
__device__ __forceinline__ void spg_px_head_wsum_partials(const SpgEccHead& hd, double* part) {
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  // (per pass over 1024 nodes: the four labels, then the four class weights, then the four sums -- the loads of the four chains used to
  //  follow each other, two dependent round trips each; the order of every sum is unchanged)
  for (int i0 = 0; i0 < hd.N; i0 += 1024) {
    int64_t t[4];
    float w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + (int)threadIdx.x + 256 * q;
      t[q] = hd.target[i < hd.N ? i : 0];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool ok = t[q] != hd.ignore_index && t[q] >= 0 && t[q] < hd.C;
      w[q] = hd.class_weight ? hd.class_weight[ok ? t[q] : 0] : 1.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + (int)threadIdx.x + 256 * q;
      if (i < hd.N && t[q] != hd.ignore_index && t[q] >= 0 && t[q] < hd.C) acc[q] += (double)w[q];
    }
  }
  spg_wave_sum4_f64(acc);
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if ((threadIdx.x & 63) == 0) part[(threadIdx.x >> 6) + 4 * q] = acc[q];
}
// the same for N <= 1024 (one pass) in two steps: the label loads are issued by `labels` (in front of other staging work), the sums
// follow in `from_labels` -- one dependent round trip behind them instead of two
__device__ __forceinline__ void spg_px_head_wsum_labels(const SpgEccHead& hd, int64_t (&t)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = (int)threadIdx.x + 256 * q;
    t[q] = hd.target[i < hd.N ? i : 0];
  }
}
__device__ __forceinline__ void spg_px_head_wsum_from_labels(const SpgEccHead& hd, const int64_t (&t)[4], double* part) {
  float w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool ok = t[q] != hd.ignore_index && t[q] >= 0 && t[q] < hd.C;
    w[q] = hd.class_weight ? hd.class_weight[ok ? t[q] : 0] : 1.f;
  }
  double acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = (int)threadIdx.x + 256 * q;
    acc[q] = 0.0;
    if (i < hd.N && t[q] != hd.ignore_index && t[q] >= 0 && t[q] < hd.C) acc[q] += (double)w[q];
  }
  spg_wave_sum4_f64(acc);
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if ((threadIdx.x & 63) == 0) part[(threadIdx.x >> 6) + 4 * q] = acc[q];
}
__device__ __forceinline__ float spg_px_head_wsum_finish(const double* part) {
  double b = 0.0;
  for (int k = 0; k < 16; ++k) b += part[k];
  return (float)b;
}

// logits of this node += W[:, col0 : col0 + 32] h, h = sh[0..31] (the wave's LDS copy of a state); lane c < C owns class c
__device__ __forceinline__ void spg_px_head_accum(const float* wc, int ldw, int col0, const float* sh, int lane, int C, float& hlog) {
  if (lane < C) {
    const f32x4* wr = reinterpret_cast<const f32x4*>(wc + lane * ldw + col0);
    const f32x4* hv = reinterpret_cast<const f32x4*>(sh);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 w = wr[q], h = hv[q];
      hlog = fmaf(h[0], w[0], hlog); hlog = fmaf(h[1], w[1], hlog); hlog = fmaf(h[2], w[2], hlog); hlog = fmaf(h[3], w[3], hlog);
    }
  }
}

// One node behind its last iteration: hlog = the finished logit of class `lane` (lanes < C).  Per element the expressions of
// spg_loss.hip (ce_fwd_bwd_kernel) except that the softmax is exp(x - lse) with lse = m + log s rounded to float32 (spg_loss.hip
// keeps m and log s apart; the two differ by ulp(m) / 2 in the exponent, round-off at the |x| < 100 of a classifier); every lane reads the node's C logits back from LDS and forms the max and the sum of the
// exponentials itself, in class order -- ce_fwd_kernel's own loops (no cross-lane reduction on the tail of the launch).
// d loss / d (module output) = W^T g: column lane + 64 j of the output per lane and j (all states at once: consecutive lanes,
// consecutive LDS words, the j-th read 256 bytes further), the classes in order.
// t: the node's class index, -1 when it carries no loss (ignore_index / out of range); w: its class weight; sq: >= 2 * 32 floats
__device__ __forceinline__ void spg_px_head_node(const SpgEccHead& hd, const float* wc, int ldw, float wsum, int i, int lane,
                                                 float hlog, float* sq, long t, float w) {
  const int C = hd.C;
  constexpr int MQ = SPG_PX_HEAD_MAXC / 4;
  if (lane < C) hd.logits[(long)i * C + lane] = hlog;
  if (lane < SPG_PX_HEAD_MAXC) sq[lane] = lane < C ? hlog : -FLT_MAX;
  spg_node_sync<true>();
  float m = -FLT_MAX;
#pragma unroll
  for (int q = 0; q < MQ; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(sq + 4 * q);
    m = fmaxf(fmaxf(fmaxf(fmaxf(m, v[0]), v[1]), v[2]), v[3]);
  }
  const float ex = lane < C ? expf(hlog - m) : 0.f;
  if (lane < SPG_PX_HEAD_MAXC) sq[SPG_PX_HEAD_MAXC + lane] = ex;
  spg_node_sync<true>();
  float ssum = 0.f;
#pragma unroll
  for (int q = 0; q < MQ; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(sq + SPG_PX_HEAD_MAXC + 4 * q);
    ssum += v[0]; ssum += v[1]; ssum += v[2]; ssum += v[3];      // (zeros beyond C)
  }
  const float l = m + logf(ssum);
  float g = 0.f;
  if (t >= 0 && lane < C) {
    const float scale = 1.f * w / (hd.reduction_mean ? wsum : 1.f);
    g = scale * (expf(hlog - l) - (lane == (int)t ? 1.f : 0.f));
  }
  if (lane < C) hd.grad_logits[(long)i * C + lane] = g;
  if (lane == 0) hd.lse[i] = l;
  spg_node_sync<true>();
  if (lane < SPG_PX_HEAD_MAXC) sq[lane] = g;
  spg_node_sync<true>();
  constexpr int NJ = SPG_PX_MAX_ITERS * 32 / 64;      // nin <= 32 (R + 1) <= 512 columns: 8 per lane
  float d[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) d[j] = 0.f;
  const float* wl = wc + lane;
  for (int c = 0; c < C; ++c) {
    const float gc = sq[c];
    const float* wr = wl + c * ldw;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (64 * j < hd.nin) d[j] = fmaf(gc, lane + 64 * j < hd.nin ? wr[64 * j] : 0.f, d[j]);      // (outer test: uniform)
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (lane + 64 * j < hd.nin) hd.grad_out[(long)i * hd.nin + lane + 64 * j] = d[j];
  spg_node_sync<true>();
}

// The loss: sum over the rows of w_t (lse - x_t) with ce_fwd_kernel's summation order (see spg_px_head_wsum_partials), by ONE
// workgroup of the launch BEHIND the one that ran the head -- a service workgroup of the persistent backward (without a spare
// CU: its workgroup 0, once its own nodes are through).  A launch boundary orders the head's stores in front of these loads;
// inside the forward launch the same sum would need agent-scope release fences in every wave: an L2 write-back each -- measured
// +38 us on a 54 us kernel.
__device__ __forceinline__ void spg_px_head_loss(const SpgEccHead& hd, double* part_l, double* part_w, int* flag) {
  if (threadIdx.x == 0) flag[0] = 0;
  __syncthreads();
  double accl[4] = {0.0, 0.0, 0.0, 0.0}, accw[4] = {0.0, 0.0, 0.0, 0.0};
  const int C = hd.C;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    for (int i = (int)threadIdx.x + 256 * q; i < hd.N; i += 1024) {
      const int64_t t = hd.target[i];
      if (t != hd.ignore_index && t >= 0 && t < C) {
        const float w = hd.class_weight ? hd.class_weight[t] : 1.f;
        accl[q] += (double)(w * (hd.lse[i] - hd.logits[(long)i * C + t]));
        accw[q] += (double)w;
      } else if (t != hd.ignore_index) {
        flag[0] = 1;      // a class index outside [0, C) that is not ignore_index: the loss becomes NaN (spg_loss.hip)
      }
    }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    for (int off = 32; off >= 1; off >>= 1) { accl[q] += __shfl_xor(accl[q], off, 64); accw[q] += __shfl_xor(accw[q], off, 64); }
    if ((threadIdx.x & 63) == 0) { part_l[(threadIdx.x >> 6) + 4 * q] = accl[q]; part_w[(threadIdx.x >> 6) + 4 * q] = accw[q]; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int k = 0; k < 16; ++k) { a += part_l[k]; b += part_w[k]; }
    *hd.wsum = (float)b;
    *hd.loss = flag[0] ? __builtin_nanf("") : (float)(hd.reduction_mean ? a / b : a);
  }
}

// The classifier's weight and bias gradient by the service workgroups of the persistent backward (CUs the recurrence leaves
// idle; measured as a job of a grouped launch: +10 us wherever it rides): dW[c][k] = sum_i g[i][c] X[i][k], db[c] = sum_i g[i][c].
// Work items of ONE wave each: a block of 64 columns over all rows -- no LDS, no synchronisation.
// dW^T block = G^T X as v_mfma_f32_16x16x4_f32 (C <= 16 classes x 16 columns x 4 rows per instruction; four column blocks share
// the G operand and one 16-byte load of X): 4 MFMAs + 2 loads per 4 rows, 2 U = 32 row groups of loads in flight (the loop is
// bound by load latency, ~2.5 us per dependent batch of 64 rows); rows in order (deterministic).  X = the module's output = the
// recurrence's states.  ~40 us per item at 1000 rows, six items on eight waves, next to a >= 75 us recurrence (a plain fma loop
// with one column per lane took ~90 us: 16 fmas + 16 broadcasts per row on one wave).  sw = this wave's index among nsw waves.
__device__ __forceinline__ void spg_px_head_wgrad(const SpgEccHead& hd, const float* __restrict__ X, long ldx, int sw, int nsw) {
  constexpr int U = 16;
  const int C = hd.C, N = hd.N, lane = threadIdx.x & 63;
  const int nb = (hd.nin + 63) / 64;
  const float* __restrict__ G = hd.grad_logits;
  const int lr = lane >> 4, lc = lane & 15;      // operand layout: row (K index) lr of the group, class / column index lc
  for (int item = sw; item < nb; item += nsw) {
    const bool with_db = item == 0 && hd.db != nullptr;      // the bias gradient = G^T 1: a fifth MFMA of the first item
    // this lane's quad of columns: element j of it is column index lc of MFMA j, i.e. D_j[c][lc] = dW[c][col0 + 4 lc + j]
    const int kq = 64 * item + 4 * lc;
    const bool xon = kq < hd.nin, gon = lc < C;      // (nin is a multiple of 32: whole quads)
    const float* xp = X + (xon ? kq : 0);
    const float* gp = G + (gon ? lc : 0);
    f32x4 acc[4], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float ga[U], gb[U];
    f32x4 xa[U], xb[U];
    auto load = [&](float (&g)[U], f32x4 (&x)[U], int i0) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long row = min(i0 + 4 * u + lr, N - 1);
        g[u] = gp[row * C];
        x[u] = *reinterpret_cast<const f32x4*>(xp + row * ldx);
      }
    };
    auto compute = [&](const float (&g)[U], const f32x4 (&x)[U], int i0) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float gv = (gon && i0 + 4 * u + lr < N) ? g[u] : 0.f;      // (rows beyond N, classes beyond C: zero products)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv, xon ? x[u][j] : 0.f, acc[j], 0, 0, 0);
        if (with_db) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(gv, 1.f, accb, 0, 0, 0);
      }
    };
    load(ga, xa, 0);
    for (int i0 = 0; i0 < N; i0 += 8 * U) {
      load(gb, xb, i0 + 4 * U);
      compute(ga, xa, i0);
      load(ga, xa, i0 + 8 * U);
      compute(gb, xb, i0 + 4 * U);
    }
    // D_j[c = 4 lr + v][lc] in acc[j][v]
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int c = 4 * lr + v;
      if (c < C && xon) *reinterpret_cast<f32x4*>(hd.dW + (long)c * hd.nin + kq) = f32x4{acc[0][v], acc[1][v], acc[2][v], acc[3][v]};
      if (with_db && c < C && lc == 0) hd.db[c] = accb[v];
    }
  }
}

// KMAX: in-edges per node whose filters stay in registers; WPC: workgroups per CU (1: 512 VGPRs per wave -- 12 filters and the
// cell's gate rows in registers; 2: 256 VGPRs -- 6 filters, gate rows read from the workgroup's LDS copy: twice the nodes per
// round).  Rounds (p.groups): wave slot s = 4 * blockIdx.x + wave owns node ptr[g] + s of group g for the whole recurrence, then
// of group g + 1, ...; a group is a union of whole connected components, so everything a node waits for belongs to its own
// group, whose waves are all resident and at this group or beyond -- no deadlock.  Every group has its own granule region.
#ifdef SPG_ATTRIBUTION
// (attribution builds only; tools/ecc_phase_timing.py) shader cycles of every node wave of the one-launch forward recurrence:
// [0 rest of the entry, 1 own-state part, 2 waiting for + gathering the neighbours, 3 filters + mean, 4 input part + publish,
//  5 head + exit, 6 waves, 7-10 inside the entry: up to the weight staging, cell weights, classifier weights + loss-weight partials,
//  barrier + gate rows]
__device__ unsigned long long spg_ecc_phase_t[12];
extern "C" int spg_ecc_phase_times(unsigned long long* out, int clear) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(spg_ecc_phase_t), sizeof(unsigned long long) * 12) != hipSuccess) return -1;
  if (clear) { unsigned long long z[12] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(spg_ecc_phase_t), z, sizeof(z)) != hipSuccess) return -1; }
  return 0;
}
#define SPG_X0() unsigned long long xt__ = __builtin_readcyclecounter(), xp__[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define SPG_XP(k) { const unsigned long long n__ = __builtin_readcyclecounter(); xp__[k] += n__ - xt__; xt__ = n__; }
#define SPG_XEND() if ((threadIdx.x & 63) == 0) { for (int k__ = 0; k__ < 6; ++k__) atomicAdd(&spg_ecc_phase_t[k__], xp__[k__]); \
    for (int k__ = 7; k__ < 11; ++k__) atomicAdd(&spg_ecc_phase_t[k__], xp__[k__]); if (xp__[4] != 0) atomicAdd(&spg_ecc_phase_t[6], 1ull); }
// the same for the one-launch backward recurrence: [0 entry (edge ids, filter loads, slot R), 1 an iteration's loads, 2 waiting for +
//  gathering the neighbours' gradients, 3 out-edge products, 4 cell backward, 5 publish, 6 waves]
__device__ unsigned long long spg_ecc_bwd_phase_t[8];
extern "C" int spg_ecc_bwd_phase_times(unsigned long long* out, int clear) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(spg_ecc_bwd_phase_t), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
  if (clear) { unsigned long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(spg_ecc_bwd_phase_t), z, sizeof(z)) != hipSuccess) return -1; }
  return 0;
}
#define SPG_XBEND() if ((threadIdx.x & 63) == 0) { for (int k__ = 0; k__ < 6; ++k__) atomicAdd(&spg_ecc_bwd_phase_t[k__], xp__[k__]); \
    if (xp__[5] != 0) atomicAdd(&spg_ecc_bwd_phase_t[6], 1ull); }
#else
#define SPG_X0()
#define SPG_XP(k)
#define SPG_XEND()
#define SPG_XBEND()
#endif

template <bool MATRIX, int KMAX, int WPC, bool GROUPS>
__global__ __launch_bounds__(256, WPC) void spg_ecc_persist_fwd_kernel(const SpgEccPersistFwd p) {
  __shared__ float sw[(2 * 96 + 32) * SPG_WLD];
  __shared__ __attribute__((aligned(16))) float lds[4][3][32];
  __shared__ __attribute__((aligned(16))) float hsb[4][SPG_PX_CH * 32];
  __shared__ int idb[4][SPG_PX_CH];
  extern __shared__ __attribute__((aligned(16))) float swc[];      // the head's classifier rows [C][nin + 4] (SpgEccHead)
  __shared__ double hd_part[16];
  SPG_X0();
  const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = blockIdx.x * 4 + wave;
  const bool with_head = p.head.W != nullptr;      // (uniform)
  // ONE round (GROUPS = false): the node's row of the graph is requested in front of the weight staging -- the first link of the
  // dependent chain row -> source ids / filters; its latency hides behind the staging loads (in-order counter: no extra wait)
  int e0_early = 0, deg_early = 0;
  float invdeg_early = 0.f;
  if constexpr (!GROUPS) {
    const int i0 = __builtin_amdgcn_readfirstlane(p.groups.ptr[0] + slot);
    const int ic = i0 < p.groups.ptr[1] ? i0 : p.groups.ptr[0];
    e0_early = p.g.rowptr[ic]; deg_early = p.g.rowptr[ic + 1] - e0_early;
    invdeg_early = p.g.invdeg[ic];
  }
  // (in front of the weight staging: in-order counter, no wait of their own.  Two workgroups per CU: no registers to spare for
  //  them -- the matrix build would spill -- so that build reads the parameter arrays per iteration as before)
  GruLaneBias cbv;
  if constexpr (WPC == 1) cbv.load(p.gru, lane0);
  const GruLaneBias* cb = WPC == 1 ? &cbv : nullptr;
  SPG_XP(7);
  spg_stage_cell_weights<96>(p.gru, sw);
  SPG_XP(8);
  const int hd_ldw = p.head.nin + 4;
  if (with_head) {
    const int nq = p.head.nin >> 2;      // (nin = 32 or 32 (R + 1): whole quads; W is 16-byte aligned -- checked by the launcher)
    const int ne = p.head.C * nq;
    const bool one_pass = p.head.reduction_mean && p.head.N <= 1024;      // (uniform)
    int64_t lab[4] = {0, 0, 0, 0};
    if (one_pass) spg_px_head_wsum_labels(p.head, lab);                    // (in flight under the classifier rows)
    const unsigned inv_nq = 0xffffffffu / (unsigned)nq + 1u;               // e / nq for e < 2^16 without a division per element
    for (int e0 = threadIdx.x; e0 < ne; e0 += 4 * 256) {      // (four loads in flight per thread, then their LDS writes)
      f32x4 v[4];
      int cc[4], qq[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = min(e0 + 256 * k, ne - 1);
        cc[k] = ne < 65536 ? (int)__umulhi((unsigned)e, inv_nq) : e / nq; qq[k] = e - cc[k] * nq;
        v[k] = *reinterpret_cast<const f32x4*>(p.head.W + (long)cc[k] * p.head.nin + 4 * qq[k]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e0 + 256 * k < ne) *reinterpret_cast<f32x4*>(swc + cc[k] * hd_ldw + 4 * qq[k]) = v[k];
    }
    if (one_pass) spg_px_head_wsum_from_labels(p.head, lab, hd_part);
    else if (p.head.reduction_mean) spg_px_head_wsum_partials(p.head, hd_part);
  }
  const unsigned base = __hip_atomic_load((spg_gu32*)p.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned spin_limit = spg_px_spin_limit(p.ctl);
  GruRowsLds wr;
  spg_gru_lds_rows<SPG_CELL_GRU>(sw, lane0, wr);
  float* sa = lds[wave][0];
  float* sh = lds[wave][1];
  float* sx = lds[wave][2];
  float* hs = hsb[wave];
  int* ids = idb[wave];
  SPG_XP(9);
  __syncthreads();            // the cell weights are in LDS; from here on the waves run on their own
  if (p.fsave_tag != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *p.fsave_tag = SPG_PX_SAVE_MAGIC;
  using Rows = typename SpgPxRows<WPC == 1>::type;
  Rows wq;                    // this lane's gate rows: in registers for all iterations (WPC == 1) or read from LDS
  spg_px_rows_init(wq, wr);
  SPG_XP(10);
  // (GROUPS = false: one round -- the loop and everything it costs in registers is compiled away)
  const int ngroups = GROUPS ? p.groups.n : 1;
#pragma nounroll
  for (int grp = 0; grp < ngroups; ++grp) {
  // (an opaque zero: the per-lane address arithmetic of a group's body must not be hoisted out of the group loop -- it would
  //  stay live across the whole body, in registers the resident filters need)
  const int lane = lane0 + spg_opaque_lane_zero();
  const int gbase = p.groups.ptr[grp];
  const int i = __builtin_amdgcn_readfirstlane(gbase + slot);      // (the wave's node as a scalar: see the backward kernel)
  if (i >= p.groups.ptr[grp + 1]) continue;
  // this group's granule region, addressed with GLOBAL node ids
  unsigned long long* gran = p.gran + ((long)grp * SPG_PX_MAX_ITERS * SPG_PX_MAX_NODES - gbase) * 32;
  spg_node_sync<true>();      // (the wave's LDS regions were last read by the previous group's final iteration)
  const int e0 = GROUPS ? p.g.rowptr[i] : e0_early, deg = GROUPS ? p.g.rowptr[i + 1] - e0 : deg_early;
  const float invdeg = GROUPS ? p.g.invdeg[i] : invdeg_early;
  // resident for all iterations: the filters of the first KMAX in-edges
  f32x4 wc[MATRIX ? KMAX : 1][4];
  float wv[KMAX];
  const int kb = lane >> 3;
  if (deg <= SPG_PX_CH && lane < deg) ids[lane] = p.g.src[e0 + lane];
  float hlog = with_head && lane < p.head.C && p.head.b != nullptr ? p.head.b[lane] : 0.f;      // the head: logit of class `lane`
  // the node's label and its class weight: wave-uniform, fetched now (two dependent loads that would sit on the tail otherwise)
  long hd_t = -1;
  float hd_w = 0.f;
  if (with_head) {
    const int iu = __builtin_amdgcn_readfirstlane(i);
    hd_t = p.head.target[iu];
    const bool ok = hd_t != p.head.ignore_index && hd_t >= 0 && hd_t < p.head.C;
    hd_w = ok ? (p.head.class_weight != nullptr ? p.head.class_weight[hd_t] : 1.f) : 0.f;
    if (!ok) hd_t = -1;
  }
  float hcur = 0.f;
  if (lane < 32) {
    const long hrow = p.h0_rows != nullptr ? p.h0_rows[i] : (long)i;
    hcur = hrow >= 0 ? p.h0[hrow * 32 + lane] : 0.f;
    p.states[(long)i * p.ldS + lane] = hcur;
    if (p.cat_all) p.out[(long)i * p.ldo + lane] = hcur;
  }
  // the filter loads go LAST (round 6): 48 KB per wave from HBM.  The vector-memory counter is in-order -- in front of the small loads
  // above (source ids, initial state, label) every use of one of those waited for all the filters; behind them the first iteration's
  // own-state part and its gather run while the filters arrive.
#pragma unroll
  for (int u = 0; u < KMAX; ++u) {
    wv[u] = 0.f;
    if (u < deg) {
      if constexpr (MATRIX) {
        const f32x4* We = reinterpret_cast<const f32x4*>(p.W + (long)(e0 + u) * 1024);
#pragma unroll
        for (int q = 0; q < 4; ++q) wc[u][q] = We[lane + 64 * q];
      } else {
        wv[u] = p.W[(long)(e0 + u) * 32 + (lane & 31)];
      }
    }
  }
  SPG_XP(0);
  for (int r = 0; r < p.R; ++r) {
    // ---- what depends on the node's own state only (input gate, W_hh h, its normalisation): BEFORE waiting for the neighbours ----
    if (lane < 32) sh[lane] = hcur;
    spg_node_sync<true>();
    GruFwdState st;
    spg_gru_hidden_part(p.gru, wq, sh, lane, st, cb);
    if (with_head && p.cat_all) spg_px_head_accum(swc, hd_ldw, 32 * r, sh, lane, p.head.C, hlog);      // the classifier's share of h^r
    // ---- aggregate over the in-edges: mean of h_src (.) W_e ----
    float a4[4] = {0.f, 0.f, 0.f, 0.f};
    SPG_XP(1);
    for (int c0 = 0; c0 < deg; c0 += SPG_PX_CH) {
      const int n = min(SPG_PX_CH, deg - c0);
      if (deg > SPG_PX_CH) {
        spg_node_sync<true>();
        if (lane < n) ids[lane] = p.g.src[e0 + c0 + lane];
      }
      spg_node_sync<true>();
      if (r == 0) spg_px_gather_plain(p.h0, 32, ids, n, lane, hs, p.h0_rows);
      else spg_px_gather_granules(gran + (long)r * SPG_PX_MAX_NODES * 32, base + (unsigned)r + 1u, ids, n, lane, hs, p.ctl, spin_limit);
      spg_node_sync<true>();
      SPG_XP(2);
      if constexpr (MATRIX) {
        if (c0 == 0) {
          // the neighbours' rows of ALL register-resident edges as one batch of LDS reads in front of the products (read under
          // each edge's own branch, every edge was an LDS round trip of its own; a node has up to KMAX of them and the
          // high-degree nodes are the ones an iteration waits for).  Rows u >= n are read too -- hs has SPG_PX_CH rows, stale
          // ones may hold anything -- and their products stay SKIPPED, not multiplied by zero.
          float xv[KMAX][4];
#pragma unroll
          for (int u = 0; u < KMAX; ++u) {
#pragma unroll
            for (int q = 0; q < 4; ++q) xv[u][q] = hs[u * 32 + kb + 8 * q];
          }
#pragma unroll
          for (int u = 0; u < KMAX; ++u) {
#pragma unroll
            for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(xv[u][q]));
          }
#pragma unroll
          for (int u = 0; u < KMAX; ++u) {
            if (u < n) {
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                a4[0] = fmaf(xv[u][q], wc[u][q][0], a4[0]); a4[1] = fmaf(xv[u][q], wc[u][q][1], a4[1]);
                a4[2] = fmaf(xv[u][q], wc[u][q][2], a4[2]); a4[3] = fmaf(xv[u][q], wc[u][q][3], a4[3]);
              }
            }
          }
        }
        for (int u = (c0 == 0 ? KMAX : 0); u < n; ++u) {      // beyond the register-resident filters: through L2
          const f32x4* We = reinterpret_cast<const f32x4*>(p.W + (long)(e0 + c0 + u) * 1024);
          f32x4 w[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) w[q] = We[lane + 64 * q];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float xv = hs[u * 32 + kb + 8 * q];
            a4[0] = fmaf(xv, w[q][0], a4[0]); a4[1] = fmaf(xv, w[q][1], a4[1]);
            a4[2] = fmaf(xv, w[q][2], a4[2]); a4[3] = fmaf(xv, w[q][3], a4[3]);
          }
        }
      } else if (lane < 32) {
        if (c0 == 0) {
          float xv[KMAX];      // (the same batch; one value per edge)
#pragma unroll
          for (int u = 0; u < KMAX; ++u) xv[u] = hs[u * 32 + lane];
#pragma unroll
          for (int u = 0; u < KMAX; ++u) asm volatile("" : "+v"(xv[u]));
#pragma unroll
          for (int u = 0; u < KMAX; ++u)
            if (u < n) a4[0] = fmaf(xv[u], wv[u], a4[0]);
        }
        for (int u = (c0 == 0 ? KMAX : 0); u < n; ++u)
          a4[0] = fmaf(hs[u * 32 + lane], p.W[(long)(e0 + c0 + u) * 32 + lane], a4[0]);
      }
    }
    if constexpr (MATRIX) {
#pragma unroll
      for (int off = 8; off <= 32; off <<= 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) a4[c] += __shfl_xor(a4[c], off, 64);
      }
      if (lane < 8) {
        sa[4 * lane + 0] = a4[0] * invdeg; sa[4 * lane + 1] = a4[1] * invdeg;
        sa[4 * lane + 2] = a4[2] * invdeg; sa[4 * lane + 3] = a4[3] * invdeg;
      }
    } else if (lane < 32) {
      sa[lane] = a4[0] * invdeg;
    }
    spg_node_sync<true>();
    SPG_XP(3);
    // ---- the input half of the GRU ----
    spg_gru_input_part<Rows, true>(p.gru, wq, sa, sx, lane, st, cb);
    if (lane < 32) {
      hcur = st.n + st.z * (hcur - st.n);      // hy = newgate + inputgate * (hidden - newgate), learning/modules.py:250
      // publish FIRST: the neighbours wait for this; everything the later kernels need follows behind it in the memory pipeline
      if (r + 1 < p.R) spg_px_store_granule(gran + ((long)(r + 1) * SPG_PX_MAX_NODES + i) * 32 + lane, base + (unsigned)r + 2u, hcur);
      p.states[(long)i * p.ldS + (long)(r + 1) * 32 + lane] = hcur;
      if (p.cat_all) p.out[(long)i * p.ldo + (long)(r + 1) * 32 + lane] = hcur;
      else if (r + 1 == p.R) p.out[(long)i * p.ldo + lane] = hcur;
      if (p.agg != nullptr) p.agg[(long)i * p.ldS + (long)r * 32 + lane] = sa[lane];
    }
    if (p.fsave != nullptr) spg_px_save_state(reinterpret_cast<f32x4*>(p.fsave) + ((long)i * p.R + r) * (SPG_PX_SAVE_F / 4) * 64 + lane, st);
    spg_node_sync<true>();      // sa / sh / sx are rewritten by the next iteration
    SPG_XP(4);
  }
  // ---- the head: classifier + cross entropy of this node, and the gradient the backward recurrence starts from ----
  if (with_head) {
    if (lane < 32) sh[lane] = hcur;
    spg_node_sync<true>();
    spg_px_head_accum(swc, hd_ldw, p.cat_all ? 32 * p.R : 0, sh, lane, p.head.C, hlog);
    const float wsum = p.head.reduction_mean ? spg_px_head_wsum_finish(hd_part) : 1.f;
    spg_px_head_node(p.head, swc, hd_ldw, wsum, i, lane, hlog, hs, hd_t, hd_w);
  }
  SPG_XP(5);
  }      // groups
  spg_px_finish(p.ctl, base, (unsigned)p.R + 2u);
  SPG_XEND();
}

template <bool MATRIX, int KMAX, int WPC, bool GROUPS>
__global__ __launch_bounds__(256, WPC) void spg_ecc_persist_bwd_kernel(const SpgEccPersistBwd p) {
  constexpr int GW = 96;
  __shared__ float sw[(2 * GW + 32) * SPG_WLD];
  __shared__ __attribute__((aligned(16))) float lds[4][4][GW];
  __shared__ __attribute__((aligned(16))) float hsb[4][SPG_PX_CH * 32];
  __shared__ int idb[4][SPG_PX_CH];
  __shared__ int eib[4][SPG_PX_CH];
  __shared__ double hd_part[2][16];
  __shared__ int hd_flag[1];
  const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = blockIdx.x * 4 + wave;
  if ((int)blockIdx.x >= p.node_wgs) {
    // ---- service workgroups (CUs the recurrence leaves idle): the head's loss; the classifier's parameter gradients ----
    const unsigned base = __hip_atomic_load((spg_gu32*)p.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int sv = (int)blockIdx.x - p.node_wgs;
    if (p.head.W != nullptr) {
      if (sv == 0) spg_px_head_loss(p.head, hd_part[0], hd_part[1], hd_flag);
      if (p.n_wgrad > 0) spg_px_head_wgrad(p.head, p.cat_all ? p.states : p.states + (long)p.R * 32, p.ldS, sv * 4 + wave, 4 * p.n_wgrad);
    }
    spg_px_finish(p.ctl, base, (unsigned)p.R + 2u);
    return;
  }
  SPG_X0();
  int b0_early = 0, odeg_early = 0;      // (see the forward kernel: the first link of row -> edge ids -> destinations -> filters)
  float invdeg_early = 0.f;
  if constexpr (!GROUPS) {
    const int j0 = __builtin_amdgcn_readfirstlane(p.groups.ptr[0] + slot);
    const int jc = j0 < p.groups.ptr[1] ? j0 : p.groups.ptr[0];
    b0_early = p.g.rev_rowptr[jc]; odeg_early = p.g.rev_rowptr[jc + 1] - b0_early;
    invdeg_early = p.g.invdeg[jc];
  }
  GruLaneBias cb;             // (the cell backward reads hh2 only)
  cb.load(p.gru, lane0);
  spg_stage_cell_weights<GW>(p.gru, sw);
  const unsigned base = __hip_atomic_load((spg_gu32*)p.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned spin_limit = spg_px_spin_limit(p.ctl);
  float* sa = lds[wave][0];        // [32] aggregate   | later dgi [96]
  float* sh = lds[wave][1];        // [32] hidden      | later dgh [96]
  float* sx = lds[wave][2];        // [32] gated input
  float* sd = lds[wave][3];        // [32] sum over the out-edges | later dpre [32]
  float* hs = hsb[wave];
  int* ids = idb[wave];
  int* eis = eib[wave];
  __syncthreads();            // cell weights staged; the waves run on their own from here
  // (GROUPS = false: one round -- the loop and everything it costs in registers is compiled away)
  const int ngroups = GROUPS ? p.groups.n : 1;
#pragma nounroll
  for (int grp = 0; grp < ngroups; ++grp) {
  const int laneg = lane0 + spg_opaque_lane_zero();      // (see the forward kernel)
  const int lane = laneg;
  const int gbase = p.groups.ptr[grp];
  // the node is the same for all lanes of the wave: as a SCALAR, its row offsets into the dozen per-node arrays of the backward are
  // scalar too (SGPR base + 32-bit lane offset) instead of 64-bit per-lane addresses that stay live across the iterations
  const int j = __builtin_amdgcn_readfirstlane(gbase + slot);
  if (j >= p.groups.ptr[grp + 1]) continue;
  unsigned long long* gran = p.gran + ((long)grp * SPG_PX_MAX_ITERS * SPG_PX_MAX_NODES - gbase) * 32;
  spg_node_sync<true>();
  const int b0 = GROUPS ? p.g.rev_rowptr[j] : b0_early, odeg = GROUPS ? p.g.rev_rowptr[j + 1] - b0 : odeg_early;
  const float invdeg = GROUPS ? p.g.invdeg[j] : invdeg_early;
  // out-edge list (edge id, destination) and the filters of the first KMAX out-edges: resident for all iterations.  The edge
  // ids first -- lane u holds the id of out-edge u, the filter loop reads it from there as a scalar -- then ALL filter loads back
  // to back, as the forward kernel issues its own (fetched one by one through the LDS list, every edge was a round trip of its own
  // into an array no cache holds, up to KMAX of them in front of the node's first gather)
  int e_l = 0;
  if (lane < odeg && (odeg <= SPG_PX_CH || lane < KMAX)) e_l = p.g.rev_eid[b0 + lane];
  int d_l = 0;
  if (odeg <= SPG_PX_CH && lane < odeg) d_l = p.g.dst[e_l];
  int ef[KMAX];
#pragma unroll
  for (int u = 0; u < KMAX; ++u) ef[u] = __builtin_amdgcn_readlane(e_l, u);
  f32x4 wc[MATRIX ? KMAX : 1][4];
  float wv[KMAX];
#pragma unroll
  for (int u = 0; u < KMAX; ++u) {
    wv[u] = 0.f;
    if (u < odeg) {
      const int e = ef[u];
      if constexpr (MATRIX) {
        const f32x4* We = reinterpret_cast<const f32x4*>(p.W + (long)e * 1024);
#pragma unroll
        for (int q = 0; q < 4; ++q) wc[u][q] = We[lane + 64 * q];
      } else {
        wv[u] = p.W[(long)e * 32 + (lane & 31)];
      }
    }
  }
  if (odeg <= SPG_PX_CH && lane < odeg) { eis[lane] = e_l; ids[lane] = d_l; }      // (read behind the iterations' own wave syncs)
  // The out-edge products pair the filters' elements ACROSS the four quads of an edge (packed multiplies): left alone, the compiler
  // rearranges every quad where it is loaded and waits for it there -- one round trip per edge again.  Behind this point the values
  // are new to it: the loads above stay a plain batch, the rearranging follows here, once, when all of them have arrived.
  if constexpr (MATRIX) {
#pragma unroll
    for (int u = 0; u < KMAX; ++u) {
#pragma unroll
      for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(wc[u][q]));
    }
  }
  // slot R of the per-iteration gradient matrices has no producer, but the deferred weight-gradient GEMMs and column sums run
  // over all N * (R + 1) rows: zero it here (the per-iteration path clears the whole 20 MB region with a memset instead)
  {
    const long r96 = (long)j * p.ld96 + (long)p.R * GW, r32 = (long)j * p.ld32 + (long)p.R * 32;
    p.dgi[r96 + lane] = 0.f; p.dgh[r96 + lane] = 0.f; p.dui[r96 + lane] = 0.f; p.duh[r96 + lane] = 0.f;
    if (lane < 32) {
      p.dgi[r96 + 64 + lane] = 0.f; p.dgh[r96 + 64 + lane] = 0.f; p.dui[r96 + 64 + lane] = 0.f; p.duh[r96 + 64 + lane] = 0.f;
      p.dpre[r32 + lane] = 0.f; p.xg[r32 + lane] = 0.f;
      p.G[(long)j * p.ldS + (long)p.R * 32 + lane] = 0.f;
    }
  }
  float dhdir = 0.f;          // direct GRU-path gradient wrt this node's state, carried from iteration to iteration (lanes 0..31)
  // did the forward keep its internals for this workspace?  (the per-iteration forward clears the tag)
  const bool saved = p.fsave != nullptr && p.fsave_tag != nullptr &&
                     __hip_atomic_load((const spg_gu32*)p.fsave_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == SPG_PX_SAVE_MAGIC;
  SPG_XP(0);
  // iterations R-1 .. 0 produce G^r; the extra pass r = -1 only forms the gradient wrt h^0
  for (int r = p.R - 1; r >= -1; --r) {
    // two workgroups per CU (256 registers per wave): the per-lane address arithmetic of an iteration must not be hoisted out of the
    // iteration loop either -- it would stay live across the whole body
    const int lane = laneg + (WPC == 2 ? spg_opaque_lane_zero() : 0);
    // Everything an iteration reads that depends on (j, r) only -- the forward's internals, its aggregate and state (phase 2 needs
    // them; one workgroup per CU: the registers are there) and the output gradient's row -- is requested here as ONE batch and first
    // used behind the gather: the loads are in flight while the wave polls.  No branch and no initialisation between them (a
    // load under `r >= 0` next to a zero for the other case made the compiler wait for every load in turn: three round trips in a
    // row in front of the first poll): the extra pass r = -1 reads the rows of iteration 0 and uses none of them, and lanes 32..63
    // read the row of lanes 0..31.
    const int rc = r < 0 ? 0 : r, l32 = lane & 31;
    f32x4 fq0, fq1, fq2;
    if (saved) {
      const f32x4* fs = reinterpret_cast<const f32x4*>(p.fsave) + ((long)j * p.R + rc) * (SPG_PX_SAVE_F / 4) * 64 + lane;
      fq0 = fs[0]; fq1 = fs[64]; fq2 = fs[128];
    }
    float a_pre, h_pre;
    if (WPC == 1) {
      a_pre = p.agg[(long)j * p.ldS + (long)rc * 32 + l32];
      h_pre = p.states[(long)j * p.ldS + (long)rc * 32 + l32];
    }
    float go = 0.f;             // (cat_all: slot r + 1 of the row; else the gradient wrt h^R, in the first pass only)
    if (p.cat_all || r == p.R - 1) go = p.grad_out[(long)j * p.ldgo + (p.cat_all ? (long)(r + 1) * 32 : 0) + l32];
    SPG_XP(1);
    // ---- phase 1: dH = d(out)/d(h^{r+1}) + dhdir + sum over the out-edges of W_e . G^{r+1}[dst] ----
    float dH = 0.f, nb = 0.f;      // (nb: the neighbours' share)
    if (r < p.R - 1) {
      float pq[4] = {0.f, 0.f, 0.f, 0.f};
      float acc = 0.f;
      for (int c0 = 0; c0 < odeg; c0 += SPG_PX_CH) {
        const int n = min(SPG_PX_CH, odeg - c0);
        if (odeg > SPG_PX_CH) {
          spg_node_sync<true>();
          if (lane < n) { const int e = p.g.rev_eid[b0 + c0 + lane]; eis[lane] = e; ids[lane] = p.g.dst[e]; }
        }
        spg_node_sync<true>();
        spg_px_gather_granules(gran + (long)(r + 1) * SPG_PX_MAX_NODES * 32, base + (unsigned)(r + 1) + 1u, ids, n, lane, hs, p.ctl, spin_limit);
        spg_node_sync<true>();
        SPG_XP(2);
        if constexpr (MATRIX) {
          if (c0 == 0) {
            // (one batch of LDS reads for all register-resident edges, products of rows u >= n skipped: see the forward kernel)
            f32x4 g4[KMAX];
#pragma unroll
            for (int u = 0; u < KMAX; ++u) g4[u] = *reinterpret_cast<const f32x4*>(hs + u * 32 + 4 * (lane & 7));
#pragma unroll
            for (int u = 0; u < KMAX; ++u) asm volatile("" : "+v"(g4[u]));
#pragma unroll
            for (int u = 0; u < KMAX; ++u) {
              if (u < n) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                  pq[q] += spg_dot4(wc[u][q], g4[u]);
              }
            }
          }
          for (int u = (c0 == 0 ? KMAX : 0); u < n; ++u) {
            const f32x4* We = reinterpret_cast<const f32x4*>(p.W + (long)eis[u] * 1024);
            f32x4 w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q] = We[lane + 64 * q];
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(hs + u * 32 + 4 * (lane & 7));
#pragma unroll
            for (int q = 0; q < 4; ++q) pq[q] += spg_dot4(w[q], g4);
          }
        } else if (lane < 32) {
          if (c0 == 0) {
            float gv[KMAX];      // (the same batch; one value per edge)
#pragma unroll
            for (int u = 0; u < KMAX; ++u) gv[u] = hs[u * 32 + lane];
#pragma unroll
            for (int u = 0; u < KMAX; ++u) asm volatile("" : "+v"(gv[u]));
#pragma unroll
            for (int u = 0; u < KMAX; ++u)
              if (u < n) acc = fmaf(wv[u], gv[u], acc);
          }
          for (int u = (c0 == 0 ? KMAX : 0); u < n; ++u) acc = fmaf(p.W[(long)eis[u] * 32 + lane], hs[u * 32 + lane], acc);
        }
      }
      if constexpr (MATRIX) {
#pragma unroll
        for (int off = 1; off <= 4; off <<= 1) {
#pragma unroll
          for (int q = 0; q < 4; ++q) pq[q] += __shfl_xor(pq[q], off, 64);
        }
        spg_node_sync<true>();
        if ((lane & 7) == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) sd[(lane >> 3) + 8 * q] = pq[q];   // input channel k = lane/8 + 8q
        }
        spg_node_sync<true>();
        if (lane < 32) nb = sd[lane];
      } else {
        nb = acc;
      }
    }
    if (lane < 32) {      // (the order of the sum as in the per-iteration kernel: (output gradient + direct path) + neighbours)
      dH = go;
      dH += dhdir;
      if (r < p.R - 1) dH += nb;
    }
    SPG_XP(3);
    if (r < 0) {
      if (lane < 32) {
        const long grow = p.gx_rows != nullptr ? p.gx_rows[j] : (long)j;      // (< 0: a node without an embedding -- nobody reads its gradient)
        if (grow >= 0) p.gx[grow * 32 + lane] = dH;
      }
      SPG_XP(5);
      break;
    }
    // ---- phase 2: GRU recompute + backward of iteration r ----
    spg_node_sync<true>();
    if (lane < 32) {
      sa[lane] = WPC == 1 ? a_pre : p.agg[(long)j * p.ldS + (long)r * 32 + lane];
      sh[lane] = WPC == 1 ? h_pre : p.states[(long)j * p.ldS + (long)r * 32 + lane];
    }
    spg_node_sync<true>();
    SpgGruBwdOut o;
    o.dgi = p.dgi + (long)r * GW; o.dgh = p.dgh + (long)r * GW; o.dui = p.dui + (long)r * GW; o.duh = p.duh + (long)r * GW;
    o.dpre = p.dpre + (long)r * 32; o.xg = p.xg + (long)r * 32; o.ld96 = p.ld96; o.ld32 = p.ld32;
    GruFwdState stf;
    if (saved) spg_px_unpack_state(fq0, fq1, fq2, stf);
    float dh_acc, da;
    spg_gru_backward_node<true, (WPC == 1 ? 24 : 16), (WPC == 1 ? 32 : 16)>(p.gru, sw, sa, sh, sx, sd, lane, true, j, dH, o, dh_acc, da, &stf, saved, &cb);
    SPG_XP(4);
    if (lane < 32) {
      dhdir = dh_acc;
      const float gc = da * invdeg;
      spg_px_store_granule(gran + ((long)r * SPG_PX_MAX_NODES + j) * 32 + lane, base + (unsigned)r + 1u, gc);
      p.G[(long)j * p.ldS + (long)r * 32 + lane] = gc;
    }
    SPG_XP(5);
  }
  }      // groups
  SPG_XBEND();
  // the loss of the head the forward launch ran (SpgEccHead): nobody on the device waits for it
  if (p.head.W != nullptr && blockIdx.x == 0 && (int)gridDim.x == p.node_wgs) spg_px_head_loss(p.head, hd_part[0], hd_part[1], hd_flag);
  spg_px_finish(p.ctl, base, (unsigned)p.R + 2u);
}


// ---- MORE NODES THAN WAVEFRONTS (round 5; VERDICT r4 missing #3): one connected component above SPG_PX_MAX_NODES nodes -------------
// A Semantic3D-scale scene is ONE component of ~10 000 superpoints: rounds of whole components cannot serve it, and the per-iteration
// launches cost ~45 us each (10 + 11 of them per step).  Iteration-major instead: the wavefronts of a launch with two workgroups per
// CU take nodes slot, slot + S, slot + 2 S, ... (S = wavefronts of the launch, <= SPG_PX_MULTI_NPW nodes each) ONE AFTER THE OTHER
// through iteration r before any of them enters r + 1.  No deadlock: a node of iteration r waits only for results of iteration r - 1,
// and every wave finishes r - 1 without waiting for anything of r.  Nothing stays in registers across nodes: filters are streamed
// (the "beyond KMAX" path of the kernels above: same arithmetic, same order), the nodes' states travel through LDS (forward: h,
// backward: the direct gradient path), the cell's internals are recomputed by the backward (no fsave: 3 KB per node and iteration).
// No head, no service workgroups, one group.  Granule region: [iteration][p.gran_nodes][32].
template <bool MATRIX>
__global__ __launch_bounds__(256, 3) void spg_ecc_persist_fwd_multi_kernel(const SpgEccPersistFwd p) {
  __shared__ float sw[(2 * 96 + 32) * SPG_WLD];
  __shared__ __attribute__((aligned(16))) float lds[4][3][32];
  __shared__ __attribute__((aligned(16))) float hsb[4][SPG_PX_CH * 32];
  __shared__ __attribute__((aligned(16))) float hlb[4][SPG_PX_MULTI_NPW][32];      // h of the wave's nodes, between iterations
  __shared__ int idb[4][SPG_PX_CH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S = (int)gridDim.x * 4, slot = (int)blockIdx.x * 4 + wave, N = p.g.N;
  GruLaneBias cb;
  cb.load(p.gru, lane);
  spg_stage_cell_weights<96>(p.gru, sw);
  const unsigned base = __hip_atomic_load((spg_gu32*)p.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned spin_limit = spg_px_spin_limit(p.ctl);
  GruRowsLds wq;
  spg_gru_lds_rows<SPG_CELL_GRU>(sw, lane, wq);
  float* sa = lds[wave][0];
  float* sh = lds[wave][1];
  float* sx = lds[wave][2];
  float* hs = hsb[wave];
  int* ids = idb[wave];
  __syncthreads();            // the cell weights are in LDS; from here on the waves run on their own
  const long GS = (long)p.gran_nodes * 32;      // granules of one iteration
  const int kb = lane >> 3;
  {      // h^0
    int k = 0;
    for (int i0 = slot; i0 < N; i0 += S, ++k) {
      const int i = __builtin_amdgcn_readfirstlane(i0);
      if (lane < 32) {
        const long hrow = p.h0_rows != nullptr ? p.h0_rows[i] : (long)i;
        const float h = hrow >= 0 ? p.h0[hrow * 32 + lane] : 0.f;
        hlb[wave][k][lane] = h;
        p.states[(long)i * p.ldS + lane] = h;
        if (p.cat_all) p.out[(long)i * p.ldo + lane] = h;
      }
    }
  }
#pragma nounroll
  for (int r = 0; r < p.R; ++r) {
    int k = 0;
#pragma nounroll
    for (int i0 = slot; i0 < N; i0 += S, ++k) {
      const int i = __builtin_amdgcn_readfirstlane(i0);
      const int e0 = p.g.rowptr[i], deg = p.g.rowptr[i + 1] - e0;
      const float invdeg = p.g.invdeg[i];
      spg_node_sync<true>();      // (the wave's LDS regions were last read by its previous node)
      float hcur = lane < 32 ? hlb[wave][k][lane] : 0.f;
      if (lane < 32) sh[lane] = hcur;
      if (deg <= SPG_PX_CH && lane < deg) ids[lane] = p.g.src[e0 + lane];
      spg_node_sync<true>();
      GruFwdState st;
      spg_gru_hidden_part(p.gru, wq, sh, lane, st, &cb);
      // ---- aggregate over the in-edges: mean of h_src (.) W_e, filters through L2 ----
      float a4[4] = {0.f, 0.f, 0.f, 0.f};
      for (int c0 = 0; c0 < deg; c0 += SPG_PX_CH) {
        const int n = min(SPG_PX_CH, deg - c0);
        if (deg > SPG_PX_CH) {
          spg_node_sync<true>();
          if (lane < n) ids[lane] = p.g.src[e0 + c0 + lane];
        }
        spg_node_sync<true>();
        if (r == 0) spg_px_gather_plain(p.h0, 32, ids, n, lane, hs, p.h0_rows);
        else spg_px_gather_granules(p.gran + (long)r * GS, base + (unsigned)r + 1u, ids, n, lane, hs, p.ctl, spin_limit);
        spg_node_sync<true>();
        if constexpr (MATRIX) {
          for (int u = 0; u < n; ++u) {
            const f32x4* We = reinterpret_cast<const f32x4*>(p.W + (long)(e0 + c0 + u) * 1024);
            f32x4 w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q] = We[lane + 64 * q];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float xv = hs[u * 32 + kb + 8 * q];
              a4[0] = fmaf(xv, w[q][0], a4[0]); a4[1] = fmaf(xv, w[q][1], a4[1]);
              a4[2] = fmaf(xv, w[q][2], a4[2]); a4[3] = fmaf(xv, w[q][3], a4[3]);
            }
          }
        } else if (lane < 32) {
          for (int u = 0; u < n; ++u) a4[0] = fmaf(hs[u * 32 + lane], p.W[(long)(e0 + c0 + u) * 32 + lane], a4[0]);
        }
      }
      if constexpr (MATRIX) {
#pragma unroll
        for (int off = 8; off <= 32; off <<= 1) {
#pragma unroll
          for (int c = 0; c < 4; ++c) a4[c] += __shfl_xor(a4[c], off, 64);
        }
        if (lane < 8) {
          sa[4 * lane + 0] = a4[0] * invdeg; sa[4 * lane + 1] = a4[1] * invdeg;
          sa[4 * lane + 2] = a4[2] * invdeg; sa[4 * lane + 3] = a4[3] * invdeg;
        }
      } else if (lane < 32) {
        sa[lane] = a4[0] * invdeg;
      }
      spg_node_sync<true>();
      spg_gru_input_part<GruRowsLds, true>(p.gru, wq, sa, sx, lane, st, &cb);
      if (lane < 32) {
        hcur = st.n + st.z * (hcur - st.n);      // learning/modules.py:250
        if (r + 1 < p.R) spg_px_store_granule(p.gran + (long)(r + 1) * GS + (long)i * 32 + lane, base + (unsigned)r + 2u, hcur);
        hlb[wave][k][lane] = hcur;
        p.states[(long)i * p.ldS + (long)(r + 1) * 32 + lane] = hcur;
        if (p.cat_all) p.out[(long)i * p.ldo + (long)(r + 1) * 32 + lane] = hcur;
        else if (r + 1 == p.R) p.out[(long)i * p.ldo + lane] = hcur;
        if (p.agg != nullptr) p.agg[(long)i * p.ldS + (long)r * 32 + lane] = sa[lane];
      }
    }
  }
  spg_px_finish(p.ctl, base, (unsigned)p.R + 2u);
}

template <bool MATRIX>
__global__ __launch_bounds__(256, 2) void spg_ecc_persist_bwd_multi_kernel(const SpgEccPersistBwd p) {
  constexpr int GW = 96;
  __shared__ float sw[(2 * GW + 32) * SPG_WLD];
  __shared__ __attribute__((aligned(16))) float lds[4][4][GW];
  __shared__ __attribute__((aligned(16))) float hsb[4][SPG_PX_CH * 32];
  __shared__ __attribute__((aligned(16))) float dhb[4][SPG_PX_MULTI_NPW][32];      // direct GRU-path gradient of the wave's nodes, between iterations
  __shared__ int idb[4][SPG_PX_CH];
  __shared__ int eib[4][SPG_PX_CH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S = (int)gridDim.x * 4, slot = (int)blockIdx.x * 4 + wave, N = p.g.N;
  spg_stage_cell_weights<GW>(p.gru, sw);
  const unsigned base = __hip_atomic_load((spg_gu32*)p.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned spin_limit = spg_px_spin_limit(p.ctl);
  float* sa = lds[wave][0];        // [32] aggregate   | later dgi [96]
  float* sh = lds[wave][1];        // [32] hidden      | later dgh [96]
  float* sx = lds[wave][2];        // [32] gated input
  float* sd = lds[wave][3];        // [32] sum over the out-edges | later dpre [32]
  float* hs = hsb[wave];
  int* ids = idb[wave];
  int* eis = eib[wave];
  __syncthreads();
  const long GS = (long)p.gran_nodes * 32;
  {      // slot R of the per-iteration gradient matrices has no producer (see the kernel above); the direct path starts from zero
    int k = 0;
    for (int i0 = slot; i0 < N; i0 += S, ++k) {
      const int j = __builtin_amdgcn_readfirstlane(i0);
      const long r96 = (long)j * p.ld96 + (long)p.R * GW, r32 = (long)j * p.ld32 + (long)p.R * 32;
      p.dgi[r96 + lane] = 0.f; p.dgh[r96 + lane] = 0.f; p.dui[r96 + lane] = 0.f; p.duh[r96 + lane] = 0.f;
      if (lane < 32) {
        p.dgi[r96 + 64 + lane] = 0.f; p.dgh[r96 + 64 + lane] = 0.f; p.dui[r96 + 64 + lane] = 0.f; p.duh[r96 + 64 + lane] = 0.f;
        p.dpre[r32 + lane] = 0.f; p.xg[r32 + lane] = 0.f;
        p.G[(long)j * p.ldS + (long)p.R * 32 + lane] = 0.f;
        dhb[wave][k][lane] = 0.f;
      }
    }
  }
#pragma nounroll
  for (int r = p.R - 1; r >= -1; --r) {
    int k = 0;
#pragma nounroll
    for (int i0 = slot; i0 < N; i0 += S, ++k) {
      const int j = __builtin_amdgcn_readfirstlane(i0);
      const int b0 = p.g.rev_rowptr[j], odeg = p.g.rev_rowptr[j + 1] - b0;
      const float invdeg = p.g.invdeg[j];
      spg_node_sync<true>();      // (the wave's LDS regions were last read by its previous node)
      // ---- phase 1: dH = d(out)/d(h^{r+1}) + direct path + sum over the out-edges of W_e . G^{r+1}[dst] ----
      float dH = 0.f;
      if (lane < 32) {
        if (p.cat_all) dH = p.grad_out[(long)j * p.ldgo + (long)(r + 1) * 32 + lane];
        else if (r == p.R - 1) dH = p.grad_out[(long)j * p.ldgo + lane];
        dH += dhb[wave][k][lane];
      }
      if (r < p.R - 1) {
        float pq[4] = {0.f, 0.f, 0.f, 0.f};
        float acc = 0.f;
        for (int c0 = 0; c0 < odeg; c0 += SPG_PX_CH) {
          const int n = min(SPG_PX_CH, odeg - c0);
          spg_node_sync<true>();
          if (lane < n) { const int e = p.g.rev_eid[b0 + c0 + lane]; eis[lane] = e; ids[lane] = p.g.dst[e]; }
          spg_node_sync<true>();
          spg_px_gather_granules(p.gran + (long)(r + 1) * GS, base + (unsigned)(r + 1) + 1u, ids, n, lane, hs, p.ctl, spin_limit);
          spg_node_sync<true>();
          if constexpr (MATRIX) {
            for (int u = 0; u < n; ++u) {
              const f32x4* We = reinterpret_cast<const f32x4*>(p.W + (long)eis[u] * 1024);
              f32x4 w[4];
#pragma unroll
              for (int q = 0; q < 4; ++q) w[q] = We[lane + 64 * q];
              const f32x4 g4 = *reinterpret_cast<const f32x4*>(hs + u * 32 + 4 * (lane & 7));
#pragma unroll
              for (int q = 0; q < 4; ++q) pq[q] += spg_dot4(w[q], g4);
            }
          } else if (lane < 32) {
            for (int u = 0; u < n; ++u) acc = fmaf(p.W[(long)eis[u] * 32 + lane], hs[u * 32 + lane], acc);
          }
        }
        if constexpr (MATRIX) {
#pragma unroll
          for (int off = 1; off <= 4; off <<= 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) pq[q] += __shfl_xor(pq[q], off, 64);
          }
          spg_node_sync<true>();
          if ((lane & 7) == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) sd[(lane >> 3) + 8 * q] = pq[q];   // input channel k = lane/8 + 8q
          }
          spg_node_sync<true>();
          if (lane < 32) dH += sd[lane];
        } else {
          dH += acc;
        }
      }
      if (r < 0) {
        if (lane < 32) {
          const long grow = p.gx_rows != nullptr ? p.gx_rows[j] : (long)j;
          if (grow >= 0) p.gx[grow * 32 + lane] = dH;
        }
        continue;
      }
      // ---- phase 2: GRU recompute + backward of iteration r ----
      spg_node_sync<true>();
      if (lane < 32) {
        sa[lane] = p.agg[(long)j * p.ldS + (long)r * 32 + lane];
        sh[lane] = p.states[(long)j * p.ldS + (long)r * 32 + lane];
      }
      spg_node_sync<true>();
      SpgGruBwdOut o;
      o.dgi = p.dgi + (long)r * GW; o.dgh = p.dgh + (long)r * GW; o.dui = p.dui + (long)r * GW; o.duh = p.duh + (long)r * GW;
      o.dpre = p.dpre + (long)r * 32; o.xg = p.xg + (long)r * 32; o.ld96 = p.ld96; o.ld32 = p.ld32;
      float dh_acc, da;
      spg_gru_backward_node<true>(p.gru, sw, sa, sh, sx, sd, lane, true, j, dH, o, dh_acc, da, nullptr);
      if (lane < 32) {
        dhb[wave][k][lane] = dh_acc;
        const float gc = da * invdeg;
        spg_px_store_granule(p.gran + (long)r * GS + (long)j * 32 + lane, base + (unsigned)r + 1u, gc);
        p.G[(long)j * p.ldS + (long)r * 32 + lane] = gc;
      }
    }
  }
  spg_px_finish(p.ctl, base, (unsigned)p.R + 2u);
}

// ---- host side: the exchange buffer and the launchers ----
// (which form a launch takes and how many workgroups: spg_px_plan.h; here only what needs the runtime)
static void* g_px_buf[SPG_MAX_DEVICES] = {nullptr};
static hipStream_t g_px_stream[SPG_MAX_DEVICES] = {nullptr};
static bool g_px_stream_set[SPG_MAX_DEVICES] = {false};
static std::mutex g_px_mutex;
#define SPG_PX_CTL_BYTES 256
static size_t px_bytes() {
  return SPG_PX_CTL_BYTES + (size_t)SPG_PX_MAX_GROUPS * SPG_PX_MAX_ITERS * SPG_PX_MAX_NODES * 32 * sizeof(unsigned long long);
}

static int px_device() {      // the current device, or -1
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < SPG_MAX_DEVICES ? dev : -1;
}
static int px_cus(int dev) {      // its CUs, asked once per device; 0: the query failed.  The caller holds g_px_mutex.
  static int cus[SPG_MAX_DEVICES] = {0};
  int n = 0;
  if (cus[dev] == 0 && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) cus[dev] = n;
  return cus[dev];
}

// returns the exchange buffer of device `dev`, or null when the persistent form must not be used for this launch.  The caller
// holds g_px_mutex.
static char* px_acquire(int dev, hipStream_t stream) {
  if (g_px_buf[dev] == nullptr) {
    void* b = nullptr;
    if (hipMalloc(&b, px_bytes()) != hipSuccess) return nullptr;
    if (hipMemset(b, 0, px_bytes()) != hipSuccess) { (void)hipFree(b); return nullptr; }
    g_px_buf[dev] = b;
  }
  {   // the test-only spin bound (spg_tune key 20) lives in the control block: ctl[4]
    static int g_px_limit[SPG_MAX_DEVICES] = {0};
    const int want = spg_tune_get(SPG_TUNE_PX_SPIN_LIMIT);
    if (want != g_px_limit[dev]) {
      const unsigned v = want > 0 ? (unsigned)want : want == -1 ? SPG_PX_SPIN_FORCED : 0u;
      if (hipMemcpy((char*)g_px_buf[dev] + 4 * sizeof(unsigned), &v, sizeof(v), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
      g_px_limit[dev] = want;
    }
  }
  // one stream per device drives the persistent launches (they serialise on it); another stream takes the safe path
  if (!g_px_stream_set[dev]) { g_px_stream[dev] = stream; g_px_stream_set[dev] = true; }
  if (g_px_stream[dev] != stream) {
    if (hipStreamQuery(g_px_stream[dev]) == hipSuccess) g_px_stream[dev] = stream;      // the old owner is idle: hand over
    else return nullptr;
  }
  return (char*)g_px_buf[dev];
}

// Workgroups per CU the iteration-major kernels REALLY get (registers, LDS; a build for another gfx target or a device whose CUs
// are partly masked gives fewer than the numbers they were written for): asked once per kernel.  A grid above what is resident
// would leave waves spinning to their bound for workgroups that cannot start.
template <class K>
static int px_occupancy(K kernel, int want) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, 0) != hipSuccess || n < 1) return 0;
  return n < want ? n : want;
}
static int px_multi_wpc(bool matrix, bool backward) {      // (the forward needs 168 registers and 52 KB of LDS: three workgroups per CU on gfx950)
  static int cache[2][2] = {{-1, -1}, {-1, -1}};
  int& c = cache[matrix ? 1 : 0][backward ? 1 : 0];
  if (c < 0) {
    if (backward) c = matrix ? px_occupancy(spg_ecc_persist_bwd_multi_kernel<true>, 2) : px_occupancy(spg_ecc_persist_bwd_multi_kernel<false>, 2);
    else c = matrix ? px_occupancy(spg_ecc_persist_fwd_multi_kernel<true>, 3) : px_occupancy(spg_ecc_persist_fwd_multi_kernel<false>, 3);
  }
  return c;
}

// The plan of launch `p` on the current device, then -- unless it declines -- the exchange buffer, and what both give of p.
// false: the per-iteration launches.
template <class P>
static bool px_prepare(P& p, bool backward, const SpgPxHeadFacts& head, hipStream_t stream, SpgPxPlan* pl) {
  std::lock_guard<std::mutex> lock(g_px_mutex);      // the one lock of a launch: CU count, buffer, stream hand-over
  const int dev = px_device(), cus = dev < 0 ? 0 : px_cus(dev);
  if (cus < 1) return false;
  const int occupancy = spg_px_groups_multi(p.groups) ? px_multi_wpc(p.matrix != 0, backward) : 0;
  *pl = spg_px_plan(p.groups, p.R, backward, cus, occupancy, spg_tune_get(SPG_TUNE_NO_PERSIST_ECC), head);
  char* buf = pl->form == SPG_PX_DECLINED ? nullptr : px_acquire(dev, stream);
  if (buf == nullptr) return false;
  p.ctl = (unsigned*)buf;
  p.gran = (unsigned long long*)(buf + SPG_PX_CTL_BYTES);
  p.node_wgs = pl->node_wgs;
  p.gran_nodes = pl->gran_nodes;
  return true;
}

// the exchange buffer of the current device; null while it has none, or without a valid current device (*no_device)
static char* px_current_buf(bool* no_device = nullptr) {
  const int dev = px_device();
  if (no_device != nullptr) *no_device = dev < 0;
  return dev < 0 ? nullptr : (char*)g_px_buf[dev];
}
// ctl[0..3] of that buffer (one blocking 16-byte copy); buf == nullptr: no buffer, nothing read
struct PxCtl { char* buf; hipError_t err; unsigned w[4]; };
static PxCtl px_read_ctl(bool* no_device = nullptr) {
  PxCtl c = {px_current_buf(no_device), hipSuccess, {0, 0, 0, 0}};
  if (c.buf != nullptr) c.err = hipMemcpy(c.w, c.buf, sizeof(c.w), hipMemcpyDeviceToHost);
  return c;
}
// zeroes the error word and the withheld-update counter (ctl[2], ctl[3]) where one of them was read as set
static hipError_t px_clear_ctl(const PxCtl& c) {
  const unsigned zero[2] = {0u, 0u};
  if (c.w[2] == 0u && c.w[3] == 0u) return hipSuccess;
  return hipMemcpy(c.buf + 2 * sizeof(unsigned), zero, sizeof(zero), hipMemcpyHostToDevice);
}

// the error word; clear: reads AND clears it (call that where the host synchronises anyway)
static int px_errors(bool clear) {
  const PxCtl c = px_read_ctl();
  if (c.buf == nullptr) return 0;
  return c.err != hipSuccess || (clear && px_clear_ctl(c) != hipSuccess) ? -1 : (int)c.w[2];
}
extern "C" int spg_ecc_persistent_errors(void) { return px_errors(false); }
extern "C" int spg_ecc_persistent_errors_clear(void) { return px_errors(true); }

// The fail-safe of the optimiser step (spg_adam_clamp_kernel, spg_api.hip): device address of the control block's error word
// (ctl[2]; ctl[3] counts the update launches that were withheld because of it), or null while the device has no exchange buffer
// (no persistent launch has run: nothing can have timed out).
unsigned* spg_px_guard_words() {
  char* buf = px_current_buf();
  return buf == nullptr ? nullptr : (unsigned*)buf + 2;
}

extern "C" int spg_ecc_persistent_status(int* errors, int* withheld, int clear) {
  if (errors) *errors = 0;
  if (withheld) *withheld = 0;
  bool no_device = false;
  const PxCtl c = px_read_ctl(&no_device);
  if (no_device) { spg_set_error("spg_ecc_persistent_status: no current device"); return -1; }
  if (c.buf == nullptr) return 0;
  hipError_t e = c.err;
  if (e == hipSuccess) {
    if (errors) *errors = (int)c.w[2];
    if (withheld) *withheld = (int)c.w[3];
    if (clear) e = px_clear_ctl(c);
  }
  if (e != hipSuccess) { spg_set_error("spg_ecc_persistent_status: %s", hipGetErrorString(e)); return (int)e; }
  return 0;
}

// KMAX of the variants: forward 12 / 6 register-resident filters (1 / 2 workgroups per CU); the backward's own working set is
// larger (gate gradients, the kept forward internals): 12 / SPG_PX_KMAX2B
template <bool MATRIX, bool GROUPS>
static void px_launch_fwd(const SpgEccPersistFwd& p, int wpc, dim3 grid, hipStream_t stream) {
  const size_t dyn = spg_px_head_lds_bytes(p.head);      // <= SPG_PX_HEAD_LDS: two workgroups per CU stay resident
  if (wpc == 1) hipLaunchKernelGGL((spg_ecc_persist_fwd_kernel<MATRIX, SPG_PX_KMAX1, 1, GROUPS>), grid, dim3(256), dyn, stream, p);
  else hipLaunchKernelGGL((spg_ecc_persist_fwd_kernel<MATRIX, SPG_PX_KMAX2, 2, GROUPS>), grid, dim3(256), dyn, stream, p);
}
template <bool MATRIX, bool GROUPS>
static void px_launch_bwd(const SpgEccPersistBwd& p, int wpc, dim3 grid, hipStream_t stream) {
  if (wpc == 1) hipLaunchKernelGGL((spg_ecc_persist_bwd_kernel<MATRIX, SPG_PX_KMAX1, 1, GROUPS>), grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((spg_ecc_persist_bwd_kernel<MATRIX, SPG_PX_KMAX2B, 2, GROUPS>), grid, dim3(256), 0, stream, p);
}

bool spg_launch_ecc_persist_fwd(SpgEccPersistFwd p, hipStream_t stream, int* err) {
  *err = 0;
  if (p.head.W != nullptr && (p.head.nin != (p.cat_all ? 32 * (p.R + 1) : 32) || p.head.C < 1 || p.head.C > SPG_PX_HEAD_MAXC ||
                              spg_px_head_lds_bytes(p.head) > SPG_PX_HEAD_LDS || p.head.N != p.g.N || !p.head.target || !p.head.logits ||
                              !p.head.grad_logits || !p.head.grad_out || !p.head.lse || !p.head.loss || !p.head.wsum ||
                              (((uintptr_t)p.head.W) & 15) != 0)) {
    spg_set_error("persistent ECC forward: the head needs nin = the module's output width, <= %d classes, <= %d bytes of rows and all of its buffers",
                  SPG_PX_HEAD_MAXC, SPG_PX_HEAD_LDS);
    *err = -1;
    return true;
  }
  SpgPxPlan pl;
  if (!px_prepare(p, false, SpgPxHeadFacts{false, false, 0}, stream, &pl)) return false;
  const dim3 grid(pl.node_wgs);
  if (pl.form == SPG_PX_ITER_MAJOR) {      // more nodes than wavefronts: no head (the caller was told: head_done stays false)
    if (p.head.W != nullptr) { spg_set_error("persistent ECC forward: no head above %d nodes in one round", SPG_PX_MAX_NODES); *err = -1; return true; }
    p.fsave = nullptr;
    if (p.matrix) hipLaunchKernelGGL(spg_ecc_persist_fwd_multi_kernel<true>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(spg_ecc_persist_fwd_multi_kernel<false>, grid, dim3(256), 0, stream, p);
  } else if (p.groups.n == 1) { if (p.matrix) px_launch_fwd<true, false>(p, pl.wpc, grid, stream); else px_launch_fwd<false, false>(p, pl.wpc, grid, stream); }
  else { if (p.matrix) px_launch_fwd<true, true>(p, pl.wpc, grid, stream); else px_launch_fwd<false, true>(p, pl.wpc, grid, stream); }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { spg_set_error("persistent ECC forward launch failed: %s", hipGetErrorString(e)); *err = (int)e; }
  return true;
}

bool spg_launch_ecc_persist_bwd(SpgEccPersistBwd p, hipStream_t stream, int* err, bool* head_wgrad_done) {
  *err = 0;
  if (head_wgrad_done != nullptr) *head_wgrad_done = false;
  const bool wgrad = p.head.dW != nullptr && head_wgrad_done != nullptr && p.head.C <= 16 && !spg_tune_get(SPG_TUNE_NO_HEAD_SERVICE) &&
                     (((uintptr_t)p.states | (uintptr_t)p.head.dW) & 15) == 0 && (p.ldS & 3) == 0;
  SpgPxPlan pl;
  if (!px_prepare(p, true, SpgPxHeadFacts{p.head.W != nullptr, wgrad, p.head.nin}, stream, &pl)) return false;
  p.n_wgrad = pl.n_wgrad;
  if (pl.n_wgrad > 0) *head_wgrad_done = true;
  const dim3 grid(pl.node_wgs + pl.service);
  if (pl.form == SPG_PX_ITER_MAJOR) {
    p.fsave = nullptr; p.fsave_tag = nullptr;
    memset(&p.head, 0, sizeof(p.head));
    if (p.matrix) hipLaunchKernelGGL(spg_ecc_persist_bwd_multi_kernel<true>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(spg_ecc_persist_bwd_multi_kernel<false>, grid, dim3(256), 0, stream, p);
  } else if (p.groups.n == 1) { if (p.matrix) px_launch_bwd<true, false>(p, pl.wpc, grid, stream); else px_launch_bwd<false, false>(p, pl.wpc, grid, stream); }
  else { if (p.matrix) px_launch_bwd<true, true>(p, pl.wpc, grid, stream); else px_launch_bwd<false, true>(p, pl.wpc, grid, stream); }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { spg_set_error("persistent ECC backward launch failed: %s", hipGetErrorString(e)); *err = (int)e; }
  return true;
}
