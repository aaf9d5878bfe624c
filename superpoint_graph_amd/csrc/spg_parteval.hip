// Evaluation of a predicted partition and the SEAL edge weights (reference supervized_partition/supervized_partition.py:248-375
// evaluate / evaluate_final, partition/provider.py:689-695 perfect_prediction, learning/metrics.py:87-108, supervized_partition/
// losses.py:119-128 compute_weights_SEAL, :168-186 mode / relax_edge_binary).  Every output is an integer or one float64
// expression of integers rounded once: the only atomics are integer ones, so the results do not depend on scheduling.
//
// Partition index (spg_partition_index):
//   pi_keys_kernel       (component, vertex) pairs; an id outside [0, n_com) is flagged and keyed n_com (behind every component);
//   rocPRIM radix sort   by component -- stable, so the vertices of one component stay in ascending id (np.flatnonzero order);
//   pi_offsets_kernel    offsets[c] = lower bound of c in the sorted components, size[c] = offsets[c + 1] - offsets[c].
// Label sums and majority (spg_component_label_majority):
//   cl_sums_kernel<LPR>  LPR = 1 ... 64 lanes per row (one lane per class); a lane group walks CL_ROWS consecutive rows of the
//                        component order with an int64 partial sum per class and adds it to sums[c] whenever the component
//                        changes: a short component is one atomic per class, a long one is split into integer partial sums;
//   cl_majority_kernel   a lane group per component: first arg-max over the classes by xor-shuffles, the component's sums into an
//                        LDS copy of the confusion matrix (column = its label), one 64-bit atomic per non-zero cell and block;
//   cl_spread_kernel     full_pred[v] = label_com[in_component[v]].
// Mode (spg_component_mode): (component << 32 | value) keys -> radix sort -> run lengths -> cm_segmax_kernel: (count << 32 |
//   2^31 - 1 - value) per run, a segmented maximum inside the wavefront (runs of one component are adjacent), one atomicMax per
//   component and wavefront: the largest count, the smallest value among equals (np.unique sorts, argmax takes the first).
// SEAL weights (spg_seal_weights): one launch over the edges.
// Relaxed indicator (spg_relax_edges): per iteration rx_mark_kernel (byte marks on both ends of every set edge; idempotent plain
//   stores) and rx_set_kernel (edges from the marks).  Mode 0 reproduces the reference including its integer indexing (see
//   rx_set_kernel); mode 1 is the symmetric rule its text describes.
// Boundary counts (spg_boundary_counts): ballots of a != 0 and b != 0 per wavefront, popcounts of their four combinations on the
//   scalar unit, block sum, one 64-bit atomic per cell and block.
#include <climits>
#include <cstring>

#include "../../include/spg_hip.h"
#include "spg_part.h"

namespace {

constexpr int PE_BLOCK = 256;
constexpr int CL_ROWS = 32;            // rows of the component order one lane group sums before it has to flush
constexpr int PE_MAX_CLASSES = 64;
constexpr int BC_MAX_BLOCKS = 2048;    // grid of the boundary counts (grid-stride): 4 atomics per block
enum { PE_ERR_COMPONENT = 1, PE_ERR_VALUE = 2 };

bool sizes_ok(long n, long n_com) { return n >= 1 && n < INT_MAX && n_com >= 1 && n_com < INT_MAX; }

// -------------------------------------------------------------------------------------------------------------------
// partition index
// -------------------------------------------------------------------------------------------------------------------
__global__ void pi_keys_kernel(const int32_t* __restrict__ in_component, long n, long n_com, unsigned* __restrict__ keys,
                               unsigned* __restrict__ vals, int32_t* __restrict__ flag) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (v < n) {
    const int c = in_component[v];
    bad = c < 0 || c >= n_com;
    keys[v] = bad ? (unsigned)n_com : (unsigned)c;
    vals[v] = (unsigned)v;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, PE_ERR_COMPONENT);
}

__device__ __forceinline__ long pe_lower_bound(const unsigned* __restrict__ keys, long lo, long hi, unsigned c) {
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (keys[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void pi_offsets_kernel(const unsigned* __restrict__ keys, long n, long n_com, int32_t* __restrict__ offsets,
                                  int32_t* __restrict__ size) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > n_com) return;
  const long lo = pe_lower_bound(keys, 0, n, (unsigned)c);
  offsets[c] = (int32_t)lo;
  if (c < n_com) size[c] = (int32_t)(pe_lower_bound(keys, lo, n, (unsigned)c + 1u) - lo);
}

struct PartitionIndexWs {      // (component, vertex) pairs: keys in / out, values in; rocPRIM scratch
  unsigned *k0, *k1, *v0;
  void* tmp; size_t tmp_bytes;
  PartitionIndexWs(Carve& w, long n) {
    k0 = w.take_n<unsigned>(n); k1 = w.take_n<unsigned>(n); v0 = w.take_n<unsigned>(n);
    tmp_bytes = radix_sort_pairs_bytes<unsigned, unsigned>(n, 0, 32);
    tmp = w.take(tmp_bytes);
  }
};

// -------------------------------------------------------------------------------------------------------------------
// label sums, majority label, confusion matrix
// -------------------------------------------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(PE_BLOCK) void cl_sums_kernel(const uint32_t* __restrict__ labels, const int32_t* __restrict__ in_component,
                                                           const int32_t* __restrict__ order, long n, int C, long n_com,
                                                           u64* __restrict__ sums) {
  const long gid = (long)blockIdx.x * PE_BLOCK + threadIdx.x;
  const long r0 = (gid / LPR) * CL_ROWS;
  const int j = (int)(gid % LPR);
  if (r0 >= n || j >= C) return;                 // (no wavefront-wide operation below)
  const long r1 = r0 + CL_ROWS < n ? r0 + CL_ROWS : n;
  u64 acc = 0;
  long cur = -1;
  for (long r = r0; r < r1; ++r) {
    const int v = order[r];
    const long c = in_component[v];
    if (c != cur) {
      if (acc != 0 && cur >= 0 && cur < n_com) atomicAdd(&sums[cur * C + j], acc);
      acc = 0; cur = c;
    }
    acc += labels[(long)v * (C + 1) + 1 + j];     // column 0 = unlabelled: left out
  }
  if (acc != 0 && cur >= 0 && cur < n_com) atomicAdd(&sums[cur * C + j], acc);
}

template <int LPR>
__global__ __launch_bounds__(PE_BLOCK) void cl_majority_kernel(const u64* __restrict__ sums, long n_com, int C, int32_t* __restrict__ label_com,
                                                               u64* __restrict__ confusion) {
  extern __shared__ u64 conf[];                   // [C, C] of this block
  for (int i = threadIdx.x; i < C * C; i += PE_BLOCK) conf[i] = 0;
  __syncthreads();
  const long gid = (long)blockIdx.x * PE_BLOCK + threadIdx.x;
  const long c = gid / LPR;
  const int j = (int)(gid % LPR);
  const bool live = c < n_com && j < C;
  const u64 s = live ? sums[c * C + j] : 0;
  // first arg-max: the larger sum wins, the smaller class among equals (a lane past C holds 0 at a larger index: never wins)
  u64 bs = s;
  int bj = j;
  for (int o = LPR / 2; o >= 1; o >>= 1) {
    const u64 os = __shfl_xor(bs, o, 64);
    const int oj = __shfl_xor(bj, o, 64);
    if (os > bs || (os == bs && oj < bj)) { bs = os; bj = oj; }
  }
  if (live && j == 0) label_com[c] = bj;
  if (live && s != 0) atomicAdd(&conf[j * C + bj], s);
  __syncthreads();
  for (int i = threadIdx.x; i < C * C; i += PE_BLOCK)
    if (conf[i] != 0) atomicAdd(&confusion[i], conf[i]);
}

__global__ void cl_spread_kernel(const int32_t* __restrict__ in_component, const int32_t* __restrict__ label_com, long n, long n_com,
                                 uint32_t* __restrict__ full_pred) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int c = in_component[v];
  full_pred[v] = (c >= 0 && c < n_com) ? (uint32_t)label_com[c] : 0u;
}

// -------------------------------------------------------------------------------------------------------------------
// mode
// -------------------------------------------------------------------------------------------------------------------
__global__ void cm_keys_kernel(const int32_t* __restrict__ in_component, const int32_t* __restrict__ values, long n, long n_com,
                               u64* __restrict__ keys, int32_t* __restrict__ flag) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int err = 0;
  if (v < n) {
    const int c = in_component[v], x = values[v];
    if (c < 0 || c >= n_com) err = PE_ERR_COMPONENT;
    else if (x < 0) err = PE_ERR_VALUE;
    keys[v] = err ? ((u64)n_com << 32) : (((u64)(unsigned)c << 32) | (u64)(unsigned)x);   // a bad entry: behind every component
  }
  for (int o = 32; o >= 1; o >>= 1) err |= __shfl_xor(err, o, 64);
  if (err != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, err);
}

__global__ __launch_bounds__(PE_BLOCK) void cm_segmax_kernel(const u64* __restrict__ ukeys, const unsigned* __restrict__ counts,
                                                             const unsigned* __restrict__ nruns, long n_com, u64* __restrict__ best) {
  const long i = (long)blockIdx.x * PE_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  unsigned comp = 0xFFFFFFFFu;                    // no run / a bad entry: a segment of its own kind that nobody writes
  u64 val = 0;
  if (i < (long)*nruns) {
    const u64 k = ukeys[i];
    if ((long)(k >> 32) < n_com) {
      comp = (unsigned)(k >> 32);
      val = ((u64)counts[i] << 32) | (u64)(0x7FFFFFFFu - (unsigned)(k & 0xFFFFFFFFu));
    }
  }
  for (int o = 1; o < 64; o <<= 1) {              // inclusive segmented maximum: the runs of one component are adjacent
    const u64 ov = __shfl_up(val, o, 64);
    const unsigned oc = __shfl_up(comp, o, 64);
    if (lane >= o && oc == comp && ov > val) val = ov;
  }
  const unsigned nc = __shfl_down(comp, 1, 64);
  if (comp != 0xFFFFFFFFu && (lane == 63 || nc != comp)) atomicMax(&best[comp], val);
}

__global__ void cm_final_kernel(const u64* __restrict__ best, long n_com, int32_t* __restrict__ freq, int32_t* __restrict__ value) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_com) return;
  const u64 b = best[c];
  freq[c] = (int32_t)(b >> 32);
  value[c] = b == 0 ? -1 : (int32_t)(0x7FFFFFFFu - (unsigned)(b & 0xFFFFFFFFu));
}

struct ComponentModeWs {
  u64 *k0, *k1, *ukeys, *best;
  unsigned *counts, *nruns;
  void* tmp; size_t tmp_bytes;
  ComponentModeWs(Carve& w, long n, long n_com) {
    k0 = w.take_n<u64>(n); k1 = w.take_n<u64>(n); ukeys = w.take_n<u64>(n);
    counts = w.take_n<unsigned>(n + 1);
    nruns = (unsigned*)w.take(256);
    best = w.take_n<u64>(n_com);
    tmp_bytes = std::max(radix_sort_keys_bytes<u64>(n, 0, 64), run_length_encode_bytes<u64, unsigned>(n));
    tmp = w.take(tmp_bytes);
  }
};

// -------------------------------------------------------------------------------------------------------------------
// SEAL weights
// -------------------------------------------------------------------------------------------------------------------
__global__ void seal_weights_kernel(const int2* __restrict__ ends, const int32_t* __restrict__ pred, const int32_t* __restrict__ size,
                                    const int32_t* __restrict__ freq, long n_com, const uint8_t* __restrict__ trans, long E, double factor,
                                    float* __restrict__ weights) {
#pragma clang fp contract(off)
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  float w = 1.f;
  if (trans[e] != 0) {
    const int2 en = ends[e];
    const int a = pred[en.x], b = pred[en.y];
    const unsigned wa = (a >= 0 && a < n_com) ? (unsigned)(size[a] - freq[a]) : 0u;       // losses.py:122-124, uint32
    const unsigned wb = (b >= 0 && b < n_com) ? (unsigned)(size[b] - freq[b]) : 0u;
    w = (float)(1.0 + (double)(wa > wb ? wa : wb) * factor);                             // :125-127: float64, one rounding
  }
  weights[e] = w;
}

// -------------------------------------------------------------------------------------------------------------------
// relaxed edge indicator
// -------------------------------------------------------------------------------------------------------------------
// losses.py:182-183.  Reference mode: edges 0 and 1 take the flags of the previous iteration's rx_set_kernel first.
__global__ void rx_mark_kernel(const int2* __restrict__ ends, uint8_t* __restrict__ relaxed, long E, const unsigned* __restrict__ flags,
                               uint8_t* __restrict__ marks) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  bool set = relaxed[e] != 0;
  if (e < 2 && !set && ((*flags >> e) & 1u) != 0) { relaxed[e] = 1; set = true; }
  if (set) {
    const int2 en = ends[e];
    marks[en.x] = 1;
    marks[en.y] = 1;
  }
}

// SYMMETRIC: an edge is set if either end is marked.  Otherwise losses.py:184-185 as numpy executes them: the uint8 vertex marks
// of the SOURCES are an integer index (values 0 and 1), so edge 1 is set if any source is marked and edge 0 if any source is
// not (flag bits 1 and 0: a block OR, then one atomicOr; applied by the next rx_mark_kernel or rx_apply_kernel), and only the
// marks of the TARGETS act as a mask.
template <bool SYMMETRIC>
__global__ __launch_bounds__(PE_BLOCK) void rx_set_kernel(const int2* __restrict__ ends, const uint8_t* __restrict__ marks, long E,
                                                          uint8_t* __restrict__ relaxed, unsigned* __restrict__ flags) {
  const long e = (long)blockIdx.x * PE_BLOCK + threadIdx.x;
  unsigned f = 0;
  if (e < E) {
    const int2 en = ends[e];
    const bool ms = marks[en.x] != 0, mt = marks[en.y] != 0;
    if (SYMMETRIC ? (ms || mt) : mt) relaxed[e] = 1;
    f = ms ? 2u : 1u;
  }
  if (!SYMMETRIC) {
    __shared__ unsigned block_or;
    if (threadIdx.x == 0) block_or = 0;
    __syncthreads();
    for (int o = 32; o >= 1; o >>= 1) f |= __shfl_xor(f, o, 64);
    if ((threadIdx.x & 63) == 0 && f != 0) atomicOr(&block_or, f);
    __syncthreads();
    if (threadIdx.x == 0 && block_or != 0) atomicOr(flags, block_or);
  }
}

__global__ void rx_apply_kernel(uint8_t* __restrict__ relaxed, long E, const unsigned* __restrict__ flags) {
  const long e = threadIdx.x;
  if (e < 2 && e < E && ((*flags >> e) & 1u) != 0) relaxed[e] = 1;
}

__global__ void pred_transition_kernel(const int2* __restrict__ ends, const int32_t* __restrict__ in_component, long E,
                                       uint8_t* __restrict__ out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int2 en = ends[e];
  out[e] = in_component[en.x] != in_component[en.y] ? 1 : 0;
}

// -------------------------------------------------------------------------------------------------------------------
// boundary counts
// -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PE_BLOCK) void bc_counts_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, long E,
                                                             u64* __restrict__ counts) {
  __shared__ u64 part[PE_BLOCK / 64][4];
  u64 c00 = 0, c01 = 0, c10 = 0, c11 = 0;         // wave-uniform: ballots and popcounts run on the scalar unit
  const long stride = (long)gridDim.x * PE_BLOCK;
  for (long base = (long)blockIdx.x * PE_BLOCK; base < E; base += stride) {
    const long e = base + threadIdx.x;
    const bool in = e < E;
    const bool pa = in && a[e] != 0, pb = in && b[e] != 0;
    const u64 mi = __ballot(in), ma = __ballot(pa), mb = __ballot(pb);
    c11 += __popcll(ma & mb);
    c10 += __popcll(ma & ~mb);
    c01 += __popcll(~ma & mb);
    c00 += __popcll(mi & ~ma & ~mb);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[wave][0] = c00; part[wave][1] = c01; part[wave][2] = c10; part[wave][3] = c11; }
  __syncthreads();
  if (threadIdx.x < 4) {
    u64 s = 0;
    for (int w = 0; w < PE_BLOCK / 64; ++w) s += part[w][threadIdx.x];
    if (s != 0) atomicAdd(&counts[threadIdx.x], s);
  }
}

struct RelaxEdgesWs {      // byte marks per vertex, flag word
  uint8_t* marks;
  unsigned* flags;
  RelaxEdgesWs(Carve& w, long n) {
    marks = w.take_n<uint8_t>(n);
    flags = (unsigned*)w.take(256);
  }
};

template <int LPR>
void launch_labels(const uint32_t* labels, const int32_t* in_component, const int32_t* order, long n, int C, long n_com, u64* sums,
                   int32_t* label_com, u64* confusion, hipStream_t st) {
  const long groups = spg_cdiv(n, CL_ROWS);
  hipLaunchKernelGGL(cl_sums_kernel<LPR>, dim3(spg_cdiv(groups * LPR, PE_BLOCK)), dim3(PE_BLOCK), 0, st, labels, in_component, order, n, C,
                     n_com, sums);
  hipLaunchKernelGGL(cl_majority_kernel<LPR>, dim3(spg_cdiv(n_com * LPR, PE_BLOCK)), dim3(PE_BLOCK), (size_t)C * C * sizeof(u64), st,
                     (const u64*)sums, n_com, C, label_com, confusion);
}

}  // namespace

extern "C" size_t spg_partition_index_workspace_bytes(long n, long n_com) {
  (void)n_com;
  Carve w;
  PartitionIndexWs l(w, std::max<long>(n, 1));
  return w.used();
}

extern "C" int spg_partition_index(const int32_t* in_component, long n, long n_com, int32_t* order, int32_t* offsets, int32_t* size,
                                   int32_t* error_flag, void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(sizes_ok(n, n_com), "1 <= n < 2^31 - 1 and 1 <= n_com < 2^31 - 1");
  SPG_CHECK_ARG(in_component && order && offsets && size && error_flag && workspace, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  Carve w(workspace, workspace_bytes);
  PartitionIndexWs l(w, n);
  unsigned *k0 = l.k0, *k1 = l.k1, *v0 = l.v0;
  void* tmp = l.tmp;
  size_t tmp_bytes = l.tmp_bytes;
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_partition_index_workspace_bytes)");
  const dim3 block(PE_BLOCK);
  hipLaunchKernelGGL(pi_keys_kernel, dim3(spg_cdiv(n, PE_BLOCK)), block, 0, st, in_component, n, n_com, k0, v0, error_flag);
  SPG_LAUNCH_CHECK();
  SPG_RP(rocprim::radix_sort_pairs(tmp, tmp_bytes, (const unsigned*)k0, k1, (const unsigned*)v0, (unsigned*)order, (size_t)n, 0,
                                   (unsigned)std::min(32, bits_of((unsigned long)n_com)), st));
  hipLaunchKernelGGL(pi_offsets_kernel, dim3(spg_cdiv(n_com + 1, PE_BLOCK)), block, 0, st, (const unsigned*)k1, n, n_com, offsets, size);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_component_label_majority(const uint32_t* labels, long n, int C, const int32_t* in_component, const int32_t* order,
                                            long n_com, int64_t* sums, int32_t* label_com, uint32_t* full_pred, int64_t* confusion,
                                            void* stream) {
  SPG_CHECK_ARG(sizes_ok(n, n_com), "1 <= n < 2^31 - 1 and 1 <= n_com < 2^31 - 1");
  SPG_CHECK_ARG(C >= 1 && C <= PE_MAX_CLASSES, "1 <= C <= 64 classes (labels is [n, C + 1])");
  SPG_CHECK_ARG(labels && in_component && order && sums && label_com && full_pred && confusion, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  SPG_RP(hipMemsetAsync(sums, 0, (size_t)n_com * C * 8, st));
  SPG_RP(hipMemsetAsync(confusion, 0, (size_t)C * C * 8, st));
#define PE_LABELS(LPR) launch_labels<LPR>(labels, in_component, order, n, C, n_com, (u64*)sums, label_com, (u64*)confusion, st)
  if (C <= 1) PE_LABELS(1);
  else if (C <= 2) PE_LABELS(2);
  else if (C <= 4) PE_LABELS(4);
  else if (C <= 8) PE_LABELS(8);
  else if (C <= 16) PE_LABELS(16);
  else if (C <= 32) PE_LABELS(32);
  else PE_LABELS(64);
#undef PE_LABELS
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(cl_spread_kernel, dim3(spg_cdiv(n, PE_BLOCK)), dim3(PE_BLOCK), 0, st, in_component, (const int32_t*)label_com, n, n_com,
                     full_pred);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spg_component_mode_workspace_bytes(long n, long n_com) {
  Carve w;
  ComponentModeWs l(w, std::max<long>(n, 1), std::max<long>(n_com, 1));
  return w.used();
}

extern "C" int spg_component_mode(const int32_t* in_component, const int32_t* values, long n, long n_com, int32_t* freq, int32_t* value,
                                  int32_t* error_flag, void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(sizes_ok(n, n_com), "1 <= n < 2^31 - 1 and 1 <= n_com < 2^31 - 1");
  SPG_CHECK_ARG(in_component && values && freq && value && error_flag && workspace, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  Carve w(workspace, workspace_bytes);
  ComponentModeWs l(w, n, n_com);
  u64 *k0 = l.k0, *k1 = l.k1, *ukeys = l.ukeys, *best = l.best;
  unsigned *counts = l.counts, *nruns = l.nruns;
  void* tmp = l.tmp;
  const size_t tmp_bytes = l.tmp_bytes;
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_component_mode_workspace_bytes)");
  const dim3 block(PE_BLOCK), gv(spg_cdiv(n, PE_BLOCK));
  SPG_RP(hipMemsetAsync(best, 0, (size_t)n_com * 8, st));
  hipLaunchKernelGGL(cm_keys_kernel, gv, block, 0, st, in_component, values, n, n_com, k0, error_flag);
  SPG_LAUNCH_CHECK();
  size_t b = tmp_bytes;
  SPG_RP(rocprim::radix_sort_keys(tmp, b, (const u64*)k0, k1, (size_t)n, 0, (unsigned)(32 + std::min(32, bits_of((unsigned long)n_com))), st));
  b = tmp_bytes;
  SPG_RP(rocprim::run_length_encode(tmp, b, (const u64*)k1, (unsigned)n, ukeys, counts, nruns, st));
  hipLaunchKernelGGL(cm_segmax_kernel, gv, block, 0, st, (const u64*)ukeys, (const unsigned*)counts, (const unsigned*)nruns, n_com, best);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(cm_final_kernel, dim3(spg_cdiv(n_com, PE_BLOCK)), block, 0, st, (const u64*)best, n_com, freq, value);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_seal_weights(const int32_t* ends, long E, long n, const int32_t* pred_in_component, const int32_t* component_size,
                                const int32_t* component_freq, long n_com, const uint8_t* is_transition, double factor, float* weights,
                                void* stream) {
  SPG_CHECK_ARG(sizes_ok(n, n_com) && E >= 0 && E < INT_MAX / 2, "1 <= n, n_com < 2^31 - 1 and 0 <= E < 2^30");
  SPG_CHECK_ARG(pred_in_component && component_size && component_freq && (E == 0 || (ends && is_transition && weights)), "bad argument");
  if (E == 0) return 0;
  hipLaunchKernelGGL(seal_weights_kernel, dim3(spg_cdiv(E, PE_BLOCK)), dim3(PE_BLOCK), 0, (hipStream_t)stream, (const int2*)ends,
                     pred_in_component, component_size, component_freq, n_com, is_transition, E, factor, weights);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spg_relax_edges_workspace_bytes(long n) {
  Carve w;
  RelaxEdgesWs l(w, std::max<long>(n, 1));
  return w.used();
}

extern "C" int spg_relax_edges(const int32_t* ends, long E, long n, const uint8_t* binary, int tolerance, int mode, uint8_t* relaxed,
                               void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(n >= 1 && n < INT_MAX && E >= 0 && E < INT_MAX / 2, "1 <= n < 2^31 - 1 and 0 <= E < 2^30");
  SPG_CHECK_ARG(tolerance >= 0, "tolerance >= 0");
  SPG_CHECK_ARG(mode == 0 || mode == 1, "mode: 0 = as the reference computes it, 1 = symmetric");
  SPG_CHECK_ARG(mode == 1 || tolerance == 0 || E >= 2, "the reference's rule writes edges 0 and 1: E >= 2");
  SPG_CHECK_ARG(workspace && (E == 0 || (ends && binary && relaxed)), "bad argument");
  if (E == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  Carve w(workspace, workspace_bytes);
  RelaxEdgesWs l(w, n);
  uint8_t* marks = l.marks;
  unsigned* flags = l.flags;
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_relax_edges_workspace_bytes)");
  SPG_RP(hipMemcpyAsync(relaxed, binary, (size_t)E, hipMemcpyDeviceToDevice, st));
  if (tolerance == 0) return 0;
  SPG_RP(hipMemsetAsync(marks, 0, (size_t)n, st));
  SPG_RP(hipMemsetAsync(flags, 0, sizeof(unsigned), st));
  const dim3 block(PE_BLOCK), ge(spg_cdiv(E, PE_BLOCK));
  for (int it = 0; it < tolerance; ++it) {
    hipLaunchKernelGGL(rx_mark_kernel, ge, block, 0, st, (const int2*)ends, relaxed, E, (const unsigned*)flags, marks);
    if (mode == 1) hipLaunchKernelGGL(rx_set_kernel<true>, ge, block, 0, st, (const int2*)ends, (const uint8_t*)marks, E, relaxed, flags);
    else hipLaunchKernelGGL(rx_set_kernel<false>, ge, block, 0, st, (const int2*)ends, (const uint8_t*)marks, E, relaxed, flags);
    SPG_LAUNCH_CHECK();
  }
  if (mode == 0) {
    hipLaunchKernelGGL(rx_apply_kernel, dim3(1), dim3(64), 0, st, relaxed, E, (const unsigned*)flags);
    SPG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int spg_pred_transition(const int32_t* ends, long E, long n, const int32_t* in_component, uint8_t* out, void* stream) {
  SPG_CHECK_ARG(n >= 1 && n < INT_MAX && E >= 0 && E < INT_MAX / 2, "1 <= n < 2^31 - 1 and 0 <= E < 2^30");
  SPG_CHECK_ARG(in_component && (E == 0 || (ends && out)), "bad argument");
  if (E == 0) return 0;
  hipLaunchKernelGGL(pred_transition_kernel, dim3(spg_cdiv(E, PE_BLOCK)), dim3(PE_BLOCK), 0, (hipStream_t)stream, (const int2*)ends, in_component,
                     E, out);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_boundary_counts(const uint8_t* a, const uint8_t* b, long E, int64_t* counts, void* stream) {
  SPG_CHECK_ARG(E >= 0 && E < INT_MAX && counts && (E == 0 || (a && b)), "bad argument");
  hipStream_t st = (hipStream_t)stream;
  SPG_RP(hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st));
  if (E == 0) return 0;
  hipLaunchKernelGGL(bc_counts_kernel, dim3(std::min(spg_cdiv(E, PE_BLOCK), BC_MAX_BLOCKS)), dim3(PE_BLOCK), 0, st, a, b, E, (u64*)counts);
  SPG_LAUNCH_CHECK();
  return 0;
}
