// l0 cut pursuit on the device: the min cut of ops.min_cut and the per-component passes of ops.cut_pursuit.
//
// Min cut (spg_mincut): synchronous push-relabel on the incidence CSR of spg_edgegraph_build.  Arc a = edge << 1 | side is the inc
// entry itself: the arc that LEAVES the vertex in whose row it stands (side 0: source -> target, side 1: target -> source), a ^ 1 is
// its reverse.  Flow model: source -> v with capacity cost1[v] (pushed in full at the start: excess), v -> sink with capacity
// cost0[v] (rsink), every edge with cap both ways; self-loops carry nothing.  One pulse is three launches:
//   mc_push_kernel     an active vertex (excess > 0, height < n + 2) pushes to the sink if it can, else along its first admissible
//                      arc in inc order; the amount goes into pushed[arc], a slot only the arc's tail writes
//   mc_gather_kernel   every vertex folds pushed[] of its arcs and their reverses into its excess and its own arcs' residuals
//   mc_relabel_kernel  an active vertex that pushed nothing takes 1 + the lowest height behind a residual arc; heights are read
//                      from one buffer and written to the other, so the pulse count does not depend on scheduling either
// Every RELABEL_EVERY pulses the host reads one status word and a level-synchronous reverse breadth-first search from the sink
// resets the heights to exact distances (n + 2: the sink cannot be reached, such a vertex never pushes again).  The last such
// search is the answer: label 1 = the vertices that reach the sink in the residual graph of a maximum preflow, the same set for every
// maximum flow.  No workgroup waits on another; every device loop runs over one vertex's incidences; the host loops are bounded by
// max_pulses and n + 1 levels.  All arithmetic is integer.
#include <climits>
#include <cstring>

#include "../../include/spg_hip.h"
#include "spg_part.h"

namespace {

constexpr int CP_BLOCK = 256;
constexpr int MC_RELABEL_EVERY = 16;      // pulses between two global relabels = pulses per status read
constexpr int MC_BFS_BATCH = 16;          // breadth-first levels per status read
constexpr int MC_LIMIT = 1 << 28;
enum { MC_ST_ERR = 0, MC_ST_PULSES = 1, MC_ST_ACTIVE = 2, MC_ST_FRONTIER = 3, MC_ST_WORDS = 4 };
enum { MC_ERR_RANGE = 1, MC_ERR_PULSES = 2 };
enum { MC_IDLE = -1, MC_TO_SINK = -2, MC_STUCK = -3 };

struct McWs {
  int32_t* status;
  int *res, *pushed, *parc, *rsink, *h0, *h1;
  long long* excess;
  McWs(Carve& w, long n, long E) {
    status = (int32_t*)w.take(256);
    res = w.take_n<int>(2 * E);
    pushed = w.take_n<int>(2 * E);
    parc = w.take_n<int>(n);
    rsink = w.take_n<int>(n);
    h0 = w.take_n<int>(n);
    h1 = w.take_n<int>(n);
    excess = w.take_n<long long>(n);
  }
};

__device__ __forceinline__ int arc_head(const int2* __restrict__ ends, unsigned a) {
  const int2 e = ends[a >> 1];
  return (a & 1u) ? e.x : e.y;
}

__global__ __launch_bounds__(CP_BLOCK) void mc_init_vertex_kernel(long n, const int64_t* __restrict__ cost0, const int64_t* __restrict__ cost1,
                                                                  long long* __restrict__ excess, int* __restrict__ rsink,
                                                                  int* __restrict__ parc, int32_t* __restrict__ status) {
  const long v = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  int bad = 0;
  if (v < n) {
    const int64_t c0 = cost0[v], c1 = cost1[v];
    bad = c0 < 0 || c0 >= MC_LIMIT || c1 < 0 || c1 >= MC_LIMIT;
    excess[v] = bad ? 0 : c1;
    rsink[v] = bad ? 0 : (int)c0;
    parc[v] = MC_IDLE;
  }
  block_report(bad, status + MC_ST_ERR, MC_ERR_RANGE);
}

__global__ __launch_bounds__(CP_BLOCK) void mc_init_edge_kernel(long E, const int2* __restrict__ ends, const int64_t* __restrict__ cap,
                                                                int* __restrict__ res, int* __restrict__ pushed, int32_t* __restrict__ status) {
  const long e = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  int bad = 0;
  if (e < E) {
    const int64_t c = cap[e];
    bad = c < 0 || c >= MC_LIMIT;
    const int2 uv = ends[e];
    const int r = (bad || uv.x == uv.y) ? 0 : (int)c;
    res[2 * e] = r; res[2 * e + 1] = r;
    pushed[2 * e] = 0; pushed[2 * e + 1] = 0;
  }
  block_report(bad, status + MC_ST_ERR, MC_ERR_RANGE);
}

__global__ __launch_bounds__(CP_BLOCK) void mc_bfs_init_kernel(long n, const int* __restrict__ rsink, int* __restrict__ h) {
  const long v = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  if (v < n) h[v] = rsink[v] > 0 ? 1 : (int)(n + 2);
}

// level k -> k + 1.  A neighbour's height read here is n + 2, k + 1 (written by this launch) or final: only an exact k counts.
__global__ __launch_bounds__(CP_BLOCK) void mc_bfs_level_kernel(long n, const int32_t* __restrict__ rowptr, const unsigned* __restrict__ inc,
                                                                const int2* __restrict__ ends, const int* __restrict__ res, int* h, int k,
                                                                int32_t* __restrict__ status) {
  const long v = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  int found = 0;
  if (v < n && h[v] == (int)(n + 2)) {
    const int end = rowptr[v + 1];
    for (int i = rowptr[v]; i < end; ++i) {
      const unsigned a = inc[i];
      if (res[a] > 0 && h[arc_head(ends, a)] == k) { found = 1; break; }
    }
    if (found) h[v] = k + 1;
  }
  block_report(found, status + MC_ST_FRONTIER, 1);
}

__global__ __launch_bounds__(CP_BLOCK) void mc_push_kernel(long n, const int32_t* __restrict__ rowptr, const unsigned* __restrict__ inc,
                                                           const int2* __restrict__ ends, const int* __restrict__ res,
                                                           const int* __restrict__ h, long long* __restrict__ excess,
                                                           int* __restrict__ rsink, int* __restrict__ pushed, int* __restrict__ parc,
                                                           int32_t* __restrict__ status, int pulse) {
  const long v = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  int active = 0;
  if (v < n) {
    const long long ex = excess[v];
    const int hv = h[v];
    int what = MC_IDLE;
    if (ex > 0 && hv < (int)(n + 2)) {
      active = 1;
      const int rs = rsink[v];
      if (rs > 0) {
        const int amount = ex < (long long)rs ? (int)ex : rs;
        excess[v] = ex - amount;
        rsink[v] = rs - amount;
        what = MC_TO_SINK;
      } else {
        what = MC_STUCK;
        const int end = rowptr[v + 1];
        for (int i = rowptr[v]; i < end; ++i) {
          const unsigned a = inc[i];
          const int r = res[a];
          if (r > 0 && hv == h[arc_head(ends, a)] + 1) {
            pushed[a] = ex < (long long)r ? (int)ex : r;
            what = (int)a;
            break;
          }
        }
      }
    }
    parc[v] = what;
  }
  active = __syncthreads_or(active);
  if (threadIdx.x == 0 && active) atomicMax(status + MC_ST_PULSES, pulse + 1);
}

__global__ __launch_bounds__(CP_BLOCK) void mc_gather_kernel(long n, const int32_t* __restrict__ rowptr, const unsigned* __restrict__ inc,
                                                             const int* __restrict__ pushed, int* __restrict__ res,
                                                             long long* __restrict__ excess) {
  const long v = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  if (v >= n) return;
  long long delta = 0;
  const int end = rowptr[v + 1];
  for (int i = rowptr[v]; i < end; ++i) {
    const unsigned a = inc[i];
    const int d = pushed[a ^ 1u] - pushed[a];
    if (d != 0) { res[a] += d; delta += d; }
  }
  if (delta != 0) excess[v] += delta;
}

__global__ __launch_bounds__(CP_BLOCK) void mc_relabel_kernel(long n, const int32_t* __restrict__ rowptr, const unsigned* __restrict__ inc,
                                                              const int2* __restrict__ ends, const int* __restrict__ res,
                                                              const int* __restrict__ hin, int* __restrict__ hout, int* __restrict__ pushed,
                                                              const int* __restrict__ parc) {
  const long v = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  if (v >= n) return;
  const int p = parc[v];
  int hv = hin[v];
  if (p >= 0) {
    pushed[p] = 0;
  } else if (p == MC_STUCK) {
    int lo = (int)(n + 2);
    const int end = rowptr[v + 1];
    for (int i = rowptr[v]; i < end; ++i) {
      const unsigned a = inc[i];
      if (res[a] > 0) lo = min(lo, hin[arc_head(ends, a)] + 1);
    }
    hv = lo;
  }
  hout[v] = hv;
}

__global__ __launch_bounds__(CP_BLOCK) void mc_probe_kernel(long n, const long long* __restrict__ excess, const int* __restrict__ h,
                                                            int32_t* __restrict__ status) {
  const long v = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  const int active = v < n && excess[v] > 0 && h[v] < (int)(n + 2);
  block_report(active, status + MC_ST_ACTIVE, 1);
}

__global__ __launch_bounds__(CP_BLOCK) void mc_label_kernel(long n, const int* __restrict__ h, uint8_t* __restrict__ label) {
  const long v = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  if (v < n) label[v] = h[v] < (int)(n + 2);
}

struct McRun {
  const int32_t* rowptr; const unsigned* inc; const int2* ends;
  long n, E;
  McWs ws;
  hipStream_t st;
  long launches = 0, levels = 0;
  dim3 gv() const { return dim3(spg_cdiv(n, CP_BLOCK)); }

  int read_status(int32_t (&host)[MC_ST_WORDS]) {
    SPG_RP(hipMemcpyAsync(host, ws.status, sizeof(host), hipMemcpyDeviceToHost, st));
    SPG_RP(hipStreamSynchronize(st));
    return 0;
  }
  // exact distances to the sink in the residual graph; at most n + 1 levels, MC_BFS_BATCH of them per status read
  int global_relabel(int* h) {
    hipLaunchKernelGGL(mc_bfs_init_kernel, gv(), dim3(CP_BLOCK), 0, st, n, (const int*)ws.rsink, h);
    SPG_LAUNCH_CHECK();
    ++launches;
    int32_t host[MC_ST_WORDS];
    for (long k = 1; k <= n + 1;) {
      SPG_RP(hipMemsetAsync(ws.status + MC_ST_FRONTIER, 0, sizeof(int32_t), st));
      for (int j = 0; j < MC_BFS_BATCH && k <= n + 1; ++j, ++k) {
        hipLaunchKernelGGL(mc_bfs_level_kernel, gv(), dim3(CP_BLOCK), 0, st, n, rowptr, inc, ends, (const int*)ws.res, h, (int)k, ws.status);
        SPG_LAUNCH_CHECK();
        ++launches; ++levels;
      }
      SPG_TRY(read_status(host));
      if (!host[MC_ST_FRONTIER]) break;
    }
    return 0;
  }
};

// ---- the per-component passes of the partition solver ----
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// W[key] += mq, S[key, :] += mq * q over the vertices with 0 <= key < K: int64, so the order cannot matter.  A wave whose lanes share
// one key (the usual case: one large component) adds once.
__global__ __launch_bounds__(CP_BLOCK) void cp_accumulate_kernel(long n, int D, long K, const int32_t* __restrict__ key,
                                                                 const int32_t* __restrict__ mq, const int32_t* __restrict__ q,
                                                                 u64* __restrict__ W, u64* __restrict__ S) {
  const long v = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  const int k = v < n ? key[v] : -1;
  const bool in = k >= 0 && k < K;
  const long long m = in ? mq[v] : 0;
  const u64 members = __ballot(in);
  if (members == 0) return;                                   // (every branch up to the per-lane adds is wave-uniform)
  const int k0 = __shfl(k, __ffsll((unsigned long long)members) - 1, 64);
  if (__all(!in || k == k0)) {
    const long long w = wave_sum_i64(m);
    if ((threadIdx.x & 63) == 0 && w != 0) atomicAdd(&W[k0], (u64)w);
    for (int d = 0; d < D; ++d) {
      const long long s = wave_sum_i64(in ? m * q[v * D + d] : 0ll);
      if ((threadIdx.x & 63) == 0 && s != 0) atomicAdd(&S[(long)k0 * D + d], (u64)s);
    }
    return;
  }
  if (!in || m == 0) return;
  atomicAdd(&W[k], (u64)m);
  for (int d = 0; d < D; ++d) {
    const long long s = m * q[v * D + d];
    if (s != 0) atomicAdd(&S[(long)k * D + d], (u64)s);
  }
}

// squared distance to row key of C in float64: dimension by dimension, left to right, each product and sum rounded on its own
__global__ __launch_bounds__(CP_BLOCK) void cp_dist_kernel(long n, int D, long K, const int32_t* __restrict__ q, const int32_t* __restrict__ key,
                                                           const double* __restrict__ C, double* __restrict__ out) {
#pragma clang fp contract(off)
  const long v = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  if (v >= n) return;
  const int k = key[v];
  double acc = 0.0;
  if (k >= 0 && k < K) {
    for (int d = 0; d < D; ++d) {
      const double diff = (double)q[v * D + d] - C[(long)k * D + d];
      const double sq = diff * diff;
      acc = acc + sq;
    }
  }
  out[v] = acc;
}

__global__ __launch_bounds__(CP_BLOCK) void cp_far_init_kernel(long K, long n, u64* __restrict__ best, int32_t* __restrict__ idx) {
  const long k = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  if (k < K) { best[k] = 0; idx[k] = (int32_t)n; }
}
// (a squared distance is >= +0.0, so its bits order as the value does)
__global__ __launch_bounds__(CP_BLOCK) void cp_far_max_kernel(long n, long K, const double* __restrict__ dist, const int32_t* __restrict__ key,
                                                              const int32_t* __restrict__ mq, u64* __restrict__ best) {
  const long v = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  if (v >= n) return;
  const int k = key[v];
  if (k >= 0 && k < K && mq[v] > 0) atomicMax(&best[k], (u64)__double_as_longlong(dist[v]));
}
__global__ __launch_bounds__(CP_BLOCK) void cp_far_idx_kernel(long n, long K, const double* __restrict__ dist, const int32_t* __restrict__ key,
                                                              const int32_t* __restrict__ mq, const u64* __restrict__ best,
                                                              int32_t* __restrict__ idx) {
  const long v = (long)blockIdx.x * CP_BLOCK + threadIdx.x;
  if (v >= n) return;
  const int k = key[v];
  if (k >= 0 && k < K && mq[v] > 0 && (u64)__double_as_longlong(dist[v]) == best[k]) atomicMin(&idx[k], (int32_t)v);
}

bool mc_sizes_ok(long n, long E) { return n >= 1 && n < 2147483645L && E >= 0 && E < (1L << 30); }

}  // namespace

extern "C" size_t spg_mincut_workspace_bytes(long n, long E) {
  Carve w;
  McWs l(w, std::max<long>(n, 1), std::max<long>(E, 0));
  return w.used();
}

extern "C" int spg_mincut(const int32_t* rowptr, const uint32_t* inc, const int32_t* ends, long E, long n, const int64_t* cap,
                          const int64_t* cost0, const int64_t* cost1, long max_pulses, uint8_t* label, int64_t* info_host,
                          void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(mc_sizes_ok(n, E), "1 <= n < 2^31 - 3 and 0 <= E < 2^30");
  SPG_CHECK_ARG(rowptr && cost0 && cost1 && label && info_host && workspace && (E == 0 || (inc && ends && cap)), "bad argument");
  SPG_CHECK_ARG(max_pulses >= 0 && max_pulses < 2147483647L, "0 <= max_pulses < 2^31 - 1");
  Carve w(workspace, workspace_bytes);
  McRun r{rowptr, inc, (const int2*)ends, n, E, McWs(w, n, E), (hipStream_t)stream};
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_mincut_workspace_bytes)");
  const McWs& ws = r.ws;
  hipStream_t st = r.st;
  const dim3 block(CP_BLOCK), gv = r.gv(), ge(spg_cdiv(std::max<long>(E, 1), CP_BLOCK));
  SPG_RP(hipMemsetAsync(ws.status, 0, MC_ST_WORDS * sizeof(int32_t), st));
  hipLaunchKernelGGL(mc_init_vertex_kernel, gv, block, 0, st, n, cost0, cost1, ws.excess, ws.rsink, ws.parc, ws.status);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(mc_init_edge_kernel, ge, block, 0, st, E, r.ends, cap, ws.res, ws.pushed, ws.status);
  SPG_LAUNCH_CHECK();
  r.launches += 2;
  int *cur = ws.h0, *nxt = ws.h1;
  SPG_TRY(r.global_relabel(cur));
  int32_t host[MC_ST_WORDS] = {0, 0, 0, 0};
  long pulses = 0;
  for (;;) {
    SPG_RP(hipMemsetAsync(ws.status + MC_ST_ACTIVE, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(mc_probe_kernel, gv, block, 0, st, n, (const long long*)ws.excess, (const int*)cur, ws.status);
    SPG_LAUNCH_CHECK();
    ++r.launches;
    SPG_TRY(r.read_status(host));
    if ((host[MC_ST_ERR] & MC_ERR_RANGE) || !host[MC_ST_ACTIVE]) break;
    if (pulses >= max_pulses) { host[MC_ST_ERR] |= MC_ERR_PULSES; break; }
    if (pulses > 0) SPG_TRY(r.global_relabel(cur));
    for (int j = 0; j < MC_RELABEL_EVERY && pulses < max_pulses; ++j, ++pulses) {
      hipLaunchKernelGGL(mc_push_kernel, gv, block, 0, st, n, rowptr, inc, r.ends, (const int*)ws.res, (const int*)cur, ws.excess, ws.rsink,
                         ws.pushed, ws.parc, ws.status, (int)pulses);
      SPG_LAUNCH_CHECK();
      hipLaunchKernelGGL(mc_gather_kernel, gv, block, 0, st, n, rowptr, inc, (const int*)ws.pushed, ws.res, ws.excess);
      SPG_LAUNCH_CHECK();
      hipLaunchKernelGGL(mc_relabel_kernel, gv, block, 0, st, n, rowptr, inc, r.ends, (const int*)ws.res, (const int*)cur, nxt, ws.pushed,
                         (const int*)ws.parc);
      SPG_LAUNCH_CHECK();
      r.launches += 3;
      std::swap(cur, nxt);
    }
  }
  if (!(host[MC_ST_ERR] & MC_ERR_RANGE)) SPG_TRY(r.global_relabel(cur));
  hipLaunchKernelGGL(mc_label_kernel, gv, block, 0, st, n, (const int*)cur, label);
  SPG_LAUNCH_CHECK();
  ++r.launches;
  info_host[0] = host[MC_ST_ERR];
  info_host[1] = host[MC_ST_PULSES];
  info_host[2] = r.launches;
  info_host[3] = r.levels;
  return 0;
}

extern "C" int spg_cp_accumulate(const int32_t* key, const int32_t* mq, const int32_t* q, long n, int D, long K, int64_t* W, int64_t* S,
                                 void* stream) {
  SPG_CHECK_ARG(n >= 1 && K >= 1 && D >= 1 && D <= SPG_CP_MAX_D && key && mq && q && W && S, "bad argument (1 <= D <= 32)");
  hipStream_t st = (hipStream_t)stream;
  SPG_RP(hipMemsetAsync(W, 0, K * sizeof(int64_t), st));
  SPG_RP(hipMemsetAsync(S, 0, K * D * sizeof(int64_t), st));
  hipLaunchKernelGGL(cp_accumulate_kernel, dim3(spg_cdiv(n, CP_BLOCK)), dim3(CP_BLOCK), 0, st, n, D, K, key, mq, q, (u64*)W, (u64*)S);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_cp_dist(const int32_t* q, const int32_t* key, const double* C, long n, int D, long K, double* out, void* stream) {
  SPG_CHECK_ARG(n >= 1 && K >= 1 && D >= 1 && D <= SPG_CP_MAX_D && q && key && C && out, "bad argument (1 <= D <= 32)");
  hipLaunchKernelGGL(cp_dist_kernel, dim3(spg_cdiv(n, CP_BLOCK)), dim3(CP_BLOCK), 0, (hipStream_t)stream, n, D, K, q, key, C, out);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_cp_farthest(const double* dist, const int32_t* key, const int32_t* mq, long n, long K, int64_t* best_bits, int32_t* idx,
                               void* stream) {
  SPG_CHECK_ARG(n >= 1 && n < 2147483647L && K >= 1 && dist && key && mq && best_bits && idx, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(CP_BLOCK), gv(spg_cdiv(n, CP_BLOCK));
  hipLaunchKernelGGL(cp_far_init_kernel, dim3(spg_cdiv(K, CP_BLOCK)), block, 0, st, K, n, (u64*)best_bits, idx);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(cp_far_max_kernel, gv, block, 0, st, n, K, dist, key, mq, (u64*)best_bits);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(cp_far_idx_kernel, gv, block, 0, st, n, K, dist, key, mq, (const u64*)best_bits, idx);
  SPG_LAUNCH_CHECK();
  return 0;
}
