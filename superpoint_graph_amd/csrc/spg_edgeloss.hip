// Graph contrastive loss of the learned (supervised) partition and its cross-partition edge weights
// (reference supervized_partition/losses.py:24-64 zhang / compute_dist / compute_loss, :130-166 compute_weights_XPART and
// libply_c.connected_comp with cutoff = 0).
//
// Edge graph (spg_edgegraph_build, once per batch):
//   eg_keys_kernel       the 2E incidences (vertex, edge << 1 | side) in edge order, side 0 = source, 1 = target; the end points as
//                        int32 pairs (an out-of-range index is flagged and clamped to 0: every later kernel stays inside its buffers);
//   rocPRIM radix sort   of the incidences by vertex -- stable, so the entries of one vertex stay in ascending edge id;
//   eg_rowptr_kernel     rowptr[v] = lower bound of v in the sorted vertices.
// Forward (spg_edge_forward): edge_fwd_kernel, one lane per edge: both embedding rows -> diff (float64 arithmetic on the float32
//   inputs, rounded once), the loss term and d term / d diff FROM THE ROUNDED diff (so that the two-piece form, diff first and the
//   loss from the stored diff later, is the same arithmetic), float64 partial sums per workgroup in a fixed tree, then
//   edge_loss_final_kernel adds the partials in a fixed order: loss1 / loss2 do not depend on scheduling.
// Backward (spg_edge_backward): edge_bwd_kernel<LPV>, LPV = 1, 2, 4, ... 64 lanes per vertex (one lane per channel): the incidences
//   of the vertex in CSR order, float64 accumulator, one store.  No atomics: bit-identical from run to run.
// Connected components (spg_connected_components): parent[v] = v; cc_link_kernel unites the end points of every active edge with
//   atomicMin on the parent array (a lane that displaces an existing parent goes on to unite the displaced one, so no link is
//   lost; every step lowers the larger of its two labels, so it ends without waiting for anybody); cc_jump_kernel shortens the
//   trees (32 ancestors per pass, ceil(log32 n) + 1 passes); the host repeats both until a link pass changes nothing (bounded).
//   parent[x] <= x always, so a root is the smallest vertex of its tree: the labels are a function of the graph alone.
//   Components are numbered by ascending root (= smallest member: Boost's order for cutoff = 0).
// Cross-partition weights (spg_xpart_weights): active = no transition and equal predicted component -> components -> a
//   (min, max) component key per transition edge -> radix sort + run lengths -> w = 1 + min(size) / count * factor in float64.
#include <climits>
#include <cstring>

#include "../../include/spg_hip.h"
#include "spg_part.h"

namespace {

constexpr int EL_BLOCK = 256;
constexpr int CC_MAX_ROUNDS = 32;      // link + jump rounds; one round completes the forest, the next one confirms it
constexpr int CC_JUMP = 32;            // ancestors a lane follows per jump pass

// -------------------------------------------------------------------------------------------------------------------
// edge graph
// -------------------------------------------------------------------------------------------------------------------
__global__ void eg_keys_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ tgt, long E, long n,
                               unsigned* __restrict__ keys, unsigned* __restrict__ vals, int2* __restrict__ ends, int32_t* __restrict__ flag) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (e < E) {
    const int64_t s = src[e], t = tgt[e];
    const bool bs = s < 0 || s >= n, bt = t < 0 || t >= n;
    bad = bs || bt;
    // a bad end point sorts behind every vertex (key n) and reads row 0 wherever it is still followed
    keys[2 * e] = bs ? (unsigned)n : (unsigned)s;
    keys[2 * e + 1] = bt ? (unsigned)n : (unsigned)t;
    vals[2 * e] = (unsigned)(2 * e);
    vals[2 * e + 1] = (unsigned)(2 * e + 1);
    ends[e] = make_int2(bs ? 0 : (int)s, bt ? 0 : (int)t);
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

__global__ void eg_rowptr_kernel(const unsigned* __restrict__ keys, long m, long n, int32_t* __restrict__ rowptr) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v > n) return;
  long lo = 0, hi = m;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if ((long)keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  rowptr[v] = (int32_t)lo;
}

struct EdgeGraphWs {      // incidences: keys in / out, values in; rocPRIM scratch
  unsigned *k0, *k1, *v0;
  void* tmp; size_t tmp_bytes;
  EdgeGraphWs(Carve& w, long E) {
    k0 = w.take_n<unsigned>(2 * E); k1 = w.take_n<unsigned>(2 * E); v0 = w.take_n<unsigned>(2 * E);
    tmp_bytes = radix_sort_pairs_bytes<unsigned, unsigned>(2 * std::max<long>(E, 1), 0, 32);
    tmp = w.take(tmp_bytes);
  }
};

// -------------------------------------------------------------------------------------------------------------------
// forward
// -------------------------------------------------------------------------------------------------------------------
enum { DIST_EUCLIDIAN = 0, DIST_INTRINSIC = 1, DIST_SCALAR = 2 };
enum { INTRA_TV = 0, INTRA_LAPLACIAN = 1, INTRA_TVH = 2 };
enum { INTER_ZHANG = 0, INTER_TVMINUS = 1 };

struct FwdArgs {
  const float* emb;            // [n, d]
  const int2* ends;            // [E]
  const uint8_t* trans;        // [E] is_transition
  const float* weights;        // [E]
  float* diff;                 // [E] written (dist) or read (loss only)
  float* dx;                   // [E] d diff / d dot, intrinsic only
  float* dl;                   // [E] d term / d diff
  double* partials;            // [blocks, 2]
  long E;
  int d, dist_type, intra, inter;
};

// losses.py:31-42 on one edge: float64 arithmetic on the float32 rows; every operation rounded on its own
template <int dist_type>
__device__ __forceinline__ void edge_diff(const float* __restrict__ a, const float* __restrict__ b, int d, float& diff, float& dx) {
#pragma clang fp contract(off)
  double acc = 0.0;
  if ((d & 3) == 0) {
    for (int c = 0; c < d; c += 4) {
      const float4 x = *reinterpret_cast<const float4*>(a + c), y = *reinterpret_cast<const float4*>(b + c);
      if (dist_type == DIST_EUCLIDIAN) {
        const double d0 = (double)x.x - (double)y.x, d1 = (double)x.y - (double)y.y, d2 = (double)x.z - (double)y.z, d3 = (double)x.w - (double)y.w;
        acc = acc + d0 * d0; acc = acc + d1 * d1; acc = acc + d2 * d2; acc = acc + d3 * d3;
      } else {
        acc = acc + (double)x.x * (double)y.x; acc = acc + (double)x.y * (double)y.y;
        acc = acc + (double)x.z * (double)y.z; acc = acc + (double)x.w * (double)y.w;
      }
    }
  } else {
    for (int c = 0; c < d; ++c) {
      if (dist_type == DIST_EUCLIDIAN) {
        const double dd = (double)a[c] - (double)b[c];
        acc = acc + dd * dd;
      } else {
        acc = acc + (double)a[c] * (double)b[c];
      }
    }
  }
  dx = 0.f;
  if (dist_type == DIST_EUCLIDIAN) {
    diff = (float)acc;
  } else if (dist_type == DIST_SCALAR) {
    diff = (float)(acc - 1.0);
  } else {
    const double smooth = 0.999;
    const double a0 = acos(smooth), a1 = acos(-smooth), x = acc * smooth;
    diff = (float)((acos(x) - a0) / (a1 - a0) * 3.141592);
    dx = (float)(-smooth / sqrt(1.0 - x * x) / (a1 - a0) * 3.141592);
  }
}

// losses.py:44-64 on one edge, from the float32 diff: term and d term / d diff.  torch's sub-gradients: clamp(min = 0) passes
// the gradient where its argument is >= 0; a negative square-root argument is NaN, as it is there.
__device__ __forceinline__ void edge_term(float diff, float weight, int t, int dist_type, int intra, int inter, double& term, double& dl) {
#pragma clang fp contract(off)
  const double x = diff, w = weight;
  term = 0.0; dl = 0.0;
  if (t == 0) {
    if (intra == INTRA_TV) {
      const double s = sqrt(x + 1e-10);
      term = w * s; dl = w * 0.5 / s;
    } else if (intra == INTRA_LAPLACIAN) {
      term = w * x; dl = w;
    } else {
      const double delta = 0.2, d2 = delta * delta, s = sqrt(1.0 + x / d2);
      term = delta * (w * (s - 1.0)); dl = delta * w * 0.5 / s / d2;
    }
  } else if (t == 1) {
    const double s = sqrt(x + 1e-10);
    if (inter == INTER_ZHANG) {
      const double beta = dist_type == DIST_INTRINSIC ? 1.0471975512 : 1.0;
      const double arg = -w * s + w * beta;
      if (arg >= 0.0) { term = arg; dl = -w * 0.5 / s; }
      else if (arg != arg) { term = arg; dl = arg; }
    } else {
      term = s * w; dl = w * 0.5 / s;
    }
  }
}

// DT: the distance type of the DO_DIST forms (compile-time: the float64 acos of 'intrinsic' stays out of the other two)
template <bool DO_DIST, bool DO_LOSS, int DT>
__global__ __launch_bounds__(EL_BLOCK) void edge_fwd_kernel(FwdArgs a) {
  const long e = (long)blockIdx.x * EL_BLOCK + threadIdx.x;
  double t1 = 0.0, t2 = 0.0;
  if (e < a.E) {
    float diff, dx;
    if (DO_DIST) {
      const int2 en = a.ends[e];
      edge_diff<DT>(a.emb + (long)en.x * a.d, a.emb + (long)en.y * a.d, a.d, diff, dx);
      a.diff[e] = diff;
      if (a.dx != nullptr) a.dx[e] = dx;
    } else {
      diff = a.diff[e];
    }
    if (DO_LOSS) {
      const int t = a.trans[e];
      double term, dl;
      edge_term(diff, a.weights[e], t, a.dist_type, a.intra, a.inter, term, dl);
      a.dl[e] = (float)dl;
      if (t == 0) t1 = term; else t2 = term;
    }
  }
  if (DO_LOSS) {
    __shared__ double lds[PART_WAVES][2];
    double t[2] = {t1, t2};
    block_reduce<PartAll<PART_SUM>>(t, lds);      // the fixed order of spg_part.h
    if (threadIdx.x == 0) {
      a.partials[2 * (long)blockIdx.x] = t[0];
      a.partials[2 * (long)blockIdx.x + 1] = t[1];
    }
  }
}

// one workgroup: lane i adds partials i, i + 256, ... in order, then a fixed tree over the 256 lanes
__global__ __launch_bounds__(EL_BLOCK) void edge_loss_final_kernel(const double* __restrict__ partials, long nb, double* __restrict__ out) {
  __shared__ double s1[EL_BLOCK], s2[EL_BLOCK];
  double r1 = 0.0, r2 = 0.0;
  for (long i = threadIdx.x; i < nb; i += EL_BLOCK) { r1 += partials[2 * i]; r2 += partials[2 * i + 1]; }
  s1[threadIdx.x] = r1; s2[threadIdx.x] = r2;
  __syncthreads();
  for (int o = EL_BLOCK / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) { s1[threadIdx.x] += s1[threadIdx.x + o]; s2[threadIdx.x] += s2[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = s1[0]; out[1] = s2[0]; }
}

// gradient of the stand-alone loss wrt diff: up[is_transition] * dl, the same float32 product the fused backward forms
__global__ void edge_loss_bwd_kernel(const float* __restrict__ dl, const uint8_t* __restrict__ trans, const float* __restrict__ up, long E,
                                     float* __restrict__ gdiff) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  gdiff[e] = __fmul_rn(up[trans[e] != 0 ? 1 : 0], dl[e]);
}

// -------------------------------------------------------------------------------------------------------------------
// backward
// -------------------------------------------------------------------------------------------------------------------
struct BwdArgs {
  const float* emb;
  const int32_t* rowptr;
  const unsigned* inc;
  const int2* ends;
  const float* dl;             // d term / d diff (fused form) or null
  const uint8_t* trans;
  const float* up;             // [2] upstream gradients of loss1, loss2 (with dl)
  const float* gdiff;          // gradient wrt diff or null
  const float* dx;             // d diff / d dot (intrinsic) or null
  float* grad;
  long n;
  int d, euclid;
};

template <int LPV>
__global__ __launch_bounds__(EL_BLOCK) void edge_bwd_kernel(BwdArgs a) {
#pragma clang fp contract(off)
  const long gid = (long)blockIdx.x * EL_BLOCK + threadIdx.x;
  const long v = gid / LPV;
  const int c = (int)(gid % LPV);
  if (v >= a.n || c >= a.d) return;
  const int d = a.d;
  const int b = a.rowptr[v], end = a.rowptr[v + 1];
  const double ev = a.emb[v * d + c];
  const float up0 = a.dl != nullptr ? a.up[0] : 0.f, up1 = a.dl != nullptr ? a.up[1] : 0.f;
  double acc = 0.0;
  for (int i = b; i < end; ++i) {
    const unsigned x = a.inc[i], e = x >> 1;
    const int2 en = a.ends[e];
    const int o = (x & 1u) ? en.x : en.y;
    float g = 0.f;
    if (a.dl != nullptr) g = __fmul_rn(a.trans[e] != 0 ? up1 : up0, a.dl[e]);
    if (a.gdiff != nullptr) g = a.dl != nullptr ? __fadd_rn(g, a.gdiff[e]) : a.gdiff[e];
    double ge = g;
    if (a.dx != nullptr) ge = ge * (double)a.dx[e];
    const double eo = a.emb[(long)o * d + c];
    acc = acc + (a.euclid ? ge * (2.0 * (ev - eo)) : ge * eo);
  }
  a.grad[v * d + c] = (float)acc;
}

// -------------------------------------------------------------------------------------------------------------------
// connected components
// -------------------------------------------------------------------------------------------------------------------
__global__ void cc_init_kernel(int* __restrict__ parent, long n) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) parent[v] = (int)v;
}

// unite the trees of both ends of every active edge.  atomicMin(&parent[hi], lo) returns what hi pointed at: hi itself = it
// was a root and is hooked now; otherwise the displaced parent and lo still have to be united.  max(p, q) falls with every
// step (parent[x] <= x), so the loop is finite whatever the other lanes do.
__global__ void cc_link_kernel(const int2* __restrict__ ends, const uint8_t* __restrict__ active, long E, int* __restrict__ parent,
                               int* __restrict__ changed) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  bool ch = false;
  if (e < E && active[e] != 0) {
    const int2 en = ends[e];
    int p = parent[en.x], q = parent[en.y];
    while (p != q) {
      const int hi = p > q ? p : q, lo = p > q ? q : p;
      const int old = atomicMin(&parent[hi], lo);
      ch = true;
      if (old == hi) break;
      p = old; q = lo;
    }
  }
  if (__any(ch) && (threadIdx.x & 63) == 0) *changed = 1;
}

// parent[v] = its ancestor CC_JUMP steps up (or the root): depth D becomes at most ceil(D / CC_JUMP)
__global__ void cc_jump_kernel(int* __restrict__ parent, long n) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  int p = parent[v];
  for (int i = 0; i < CC_JUMP; ++i) {
    const int pp = parent[p];
    if (pp == p) break;
    p = pp;
  }
  parent[v] = p;
}

__global__ void cc_roots_kernel(const int* __restrict__ parent, long n, unsigned* __restrict__ isroot, int32_t* __restrict__ size) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v > n) return;
  isroot[v] = (v < n && parent[v] == (int)v) ? 1u : 0u;
  if (v < n) size[v] = 0;
}

__global__ void cc_label_kernel(const int* __restrict__ parent, const unsigned* __restrict__ rank, long n, int32_t* __restrict__ in_component,
                                int32_t* __restrict__ size, int32_t* __restrict__ n_components) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int c = (int)rank[parent[v]];
  in_component[v] = c;
  atomicAdd(&size[c], 1);                   // integer counts: the same whatever the order
  if (v == 0) *n_components = (int32_t)rank[n];
}

struct CcWs {
  int *changed, *parent;
  unsigned *isroot, *rank;
  void* tmp; size_t tmp_bytes;
  CcWs(Carve& w, long n) {
    changed = (int*)w.take(256);
    parent = w.take_n<int>(n);
    isroot = w.take_n<unsigned>(n + 1);
    rank = w.take_n<unsigned>(n + 1);
    tmp_bytes = exclusive_scan_bytes<unsigned>(n + 1);
    tmp = w.take(tmp_bytes);
  }
};

// (the caller has carved and checked ws)
int cc_run(const int2* ends, const uint8_t* active, long E, long n, int32_t* in_component, int32_t* component_size, int32_t* n_components,
           const CcWs& ws, hipStream_t st) {
  int *changed = ws.changed, *parent = ws.parent;
  unsigned *isroot = ws.isroot, *rank = ws.rank;
  void* tmp = ws.tmp;
  size_t tmp_bytes = ws.tmp_bytes;
  const dim3 block(EL_BLOCK), gv(spg_cdiv(n, EL_BLOCK)), ge(spg_cdiv(std::max<long>(E, 1), EL_BLOCK));
  hipLaunchKernelGGL(cc_init_kernel, gv, block, 0, st, parent, n);
  SPG_LAUNCH_CHECK();
  const int passes = (bits_of((unsigned long)n) + 4) / 5 + 1;
  bool settled = E == 0;
  for (int round = 0; round < CC_MAX_ROUNDS && !settled; ++round) {
    SPG_RP(hipMemsetAsync(changed, 0, sizeof(int), st));
    hipLaunchKernelGGL(cc_link_kernel, ge, block, 0, st, ends, active, E, parent, changed);
    SPG_LAUNCH_CHECK();
    for (int p = 0; p < passes; ++p) {
      hipLaunchKernelGGL(cc_jump_kernel, gv, block, 0, st, parent, n);
      SPG_LAUNCH_CHECK();
    }
    int h = 0;
    SPG_RP(hipMemcpyAsync(&h, changed, sizeof(int), hipMemcpyDeviceToHost, st));
    SPG_RP(hipStreamSynchronize(st));
    settled = h == 0;
  }
  if (!settled) {
    spg_set_error("%s:%d: connected components did not settle within %d rounds", __FILE__, __LINE__, CC_MAX_ROUNDS);
    return -2;
  }
  hipLaunchKernelGGL(cc_roots_kernel, dim3(spg_cdiv(n + 1, EL_BLOCK)), block, 0, st, (const int*)parent, n, isroot, component_size);
  SPG_LAUNCH_CHECK();
  SPG_RP(rocprim::exclusive_scan(tmp, tmp_bytes, (const unsigned*)isroot, rank, 0u, (size_t)(n + 1), rocprim::plus<unsigned>(), st));
  hipLaunchKernelGGL(cc_label_kernel, gv, block, 0, st, (const int*)parent, (const unsigned*)rank, n, in_component, component_size, n_components);
  SPG_LAUNCH_CHECK();
  return 0;
}

// -------------------------------------------------------------------------------------------------------------------
// cross-partition weights
// -------------------------------------------------------------------------------------------------------------------
__global__ void xp_active_kernel(const int2* __restrict__ ends, const int32_t* __restrict__ pred, const uint8_t* __restrict__ trans, long E,
                                 uint8_t* __restrict__ active) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int2 en = ends[e];
  active[e] = (trans[e] == 0 && pred[en.x] == pred[en.y]) ? 1 : 0;
}

__device__ __forceinline__ u64 xp_key(const int2 en, const int32_t* __restrict__ comp) {
  const unsigned a = (unsigned)comp[en.x], b = (unsigned)comp[en.y];
  return ((u64)(a < b ? a : b) << 32) | (u64)(a < b ? b : a);
}

__global__ void xp_keys_kernel(const int2* __restrict__ ends, const int32_t* __restrict__ comp, const uint8_t* __restrict__ trans, long E,
                               u64* __restrict__ keys) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  keys[e] = trans[e] != 0 ? xp_key(ends[e], comp) : ~0ull;       // no transition: behind every pair, never looked up
}

__global__ void xp_weights_kernel(const int2* __restrict__ ends, const int32_t* __restrict__ comp, const int32_t* __restrict__ size,
                                  const uint8_t* __restrict__ trans, long E, const u64* __restrict__ ukeys, const unsigned* __restrict__ counts,
                                  const unsigned* __restrict__ nruns, double factor, float* __restrict__ weights) {
#pragma clang fp contract(off)
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  float w = 1.f;
  if (trans[e] != 0) {
    const int2 en = ends[e];
    const u64 key = xp_key(en, comp);
    unsigned lo = 0, hi = *nruns;
    while (lo < hi) {
      const unsigned mid = (lo + hi) >> 1;
      if (ukeys[mid] < key) lo = mid + 1; else hi = mid;
    }
    const int sa = size[comp[en.x]], sb = size[comp[en.y]];
    const double m = (double)(sa < sb ? sa : sb), cnt = (double)counts[lo];
    const double add = (m / cnt) * factor;         // losses.py:153-154, float64; one rounding to float32 (:158)
    w = (float)(1.0 + add);
  }
  weights[e] = w;
}

struct XpartWs {      // E >= 1 here (an empty graph is laid out as one edge)
  CcWs cc;
  uint8_t* active;
  u64 *k0, *k1, *ukeys;
  unsigned *counts, *nruns;
  void* tmp; size_t tmp_bytes;
  XpartWs(Carve& w, long n, long E) : cc(w, n) {
    active = w.take_n<uint8_t>(E);
    k0 = w.take_n<u64>(E); k1 = w.take_n<u64>(E); ukeys = w.take_n<u64>(E);
    counts = w.take_n<unsigned>(E + 1);
    nruns = (unsigned*)w.take(256);
    tmp_bytes = std::max(radix_sort_keys_bytes<u64>(E, 0, 64), run_length_encode_bytes<u64, unsigned>(E));
    tmp = w.take(tmp_bytes);
  }
};

// per-workgroup partial sums of the forward: [blocks, 2] float64
struct EdgeForwardWs {
  double* partials;
  EdgeForwardWs(Carve& w, long E) { partials = w.take_n<double>((size_t)spg_cdiv(std::max<long>(E, 1), EL_BLOCK) * 2); }
};

template <int LPV>
void launch_bwd(const BwdArgs& a, hipStream_t st) {
  const long threads = a.n * LPV;
  hipLaunchKernelGGL(edge_bwd_kernel<LPV>, dim3(spg_cdiv(threads, EL_BLOCK)), dim3(EL_BLOCK), 0, st, a);
}

bool sizes_ok(long n, long E) { return n >= 1 && E >= 0 && n < INT_MAX && E < INT_MAX / 2; }

}  // namespace

extern "C" size_t spg_edgegraph_workspace_bytes(long n, long E) {
  (void)n;
  Carve w;
  EdgeGraphWs l(w, std::max<long>(E, 0));
  return w.used();
}

extern "C" int spg_edgegraph_build(const int64_t* src, const int64_t* tgt, long E, long n, int32_t* rowptr, uint32_t* inc, int32_t* ends,
                                   int32_t* error_flag, void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(rowptr && error_flag && (E == 0 || (src && tgt && inc && ends && workspace)), "bad argument");
  SPG_CHECK_ARG(sizes_ok(n, E), "1 <= n < 2^31 - 1 and 0 <= E < 2^30 (an incidence is edge << 1 | side in 32 bits)");
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(EL_BLOCK);
  if (E == 0) {
    SPG_RP(hipMemsetAsync(error_flag, 0, sizeof(int32_t), st));
    SPG_RP(hipMemsetAsync(rowptr, 0, (size_t)(n + 1) * 4, st));
    return 0;
  }
  Carve w(workspace, workspace_bytes);
  EdgeGraphWs l(w, E);
  unsigned *k0 = l.k0, *k1 = l.k1, *v0 = l.v0;
  void* tmp = l.tmp;
  size_t tmp_bytes = l.tmp_bytes;
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_edgegraph_workspace_bytes)");      // (before anything is written)
  SPG_RP(hipMemsetAsync(error_flag, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(eg_keys_kernel, dim3(spg_cdiv(E, EL_BLOCK)), block, 0, st, src, tgt, E, n, k0, v0, (int2*)ends, error_flag);
  SPG_LAUNCH_CHECK();
  SPG_RP(rocprim::radix_sort_pairs(tmp, tmp_bytes, (const unsigned*)k0, k1, (const unsigned*)v0, (unsigned*)inc, (size_t)(2 * E), 0,
                                   (unsigned)bits_of((unsigned long)n), st));
  hipLaunchKernelGGL(eg_rowptr_kernel, dim3(spg_cdiv(n + 1, EL_BLOCK)), block, 0, st, (const unsigned*)k1, 2 * E, n, rowptr);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spg_edge_forward_workspace_bytes(long E) {
  Carve w;
  EdgeForwardWs l(w, E);
  return w.used();
}

extern "C" int spg_edge_forward(int mode, const float* emb, long n, int d, const int32_t* ends, long E, int dist_type, int intra, int inter,
                                const uint8_t* is_transition, const float* weights, float* diff, float* dx, float* dl, double* loss_out,
                                void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(mode >= 1 && mode <= 3, "mode: 1 = diff, 2 = loss from diff, 3 = both");
  SPG_CHECK_ARG(sizes_ok(n, E), "1 <= n < 2^31 - 1 and 0 <= E < 2^30");
  SPG_CHECK_ARG(dist_type >= DIST_EUCLIDIAN && dist_type <= DIST_SCALAR, "dist_type: 0 euclidian, 1 intrinsic, 2 scalar");
  const bool do_dist = mode & 1, do_loss = mode & 2;
  double* partials = nullptr;
  if (do_dist) {
    SPG_CHECK_ARG(d >= 1 && d <= 64, "1 <= d <= 64");
    SPG_CHECK_ARG(E == 0 || (emb && ends && diff), "bad argument");
    SPG_CHECK_ARG(dist_type != DIST_INTRINSIC || E == 0 || dx, "intrinsic needs dx");
    SPG_CHECK_ARG((d & 3) != 0 || (((uintptr_t)emb) & 15) == 0, "emb must be 16-byte aligned");
  }
  if (do_loss) {
    SPG_CHECK_ARG(intra >= INTRA_TV && intra <= INTRA_TVH && inter >= INTER_ZHANG && inter <= INTER_TVMINUS, "intra: 0 tv, 1 laplacian, 2 TVH; inter: 0 zhang, 1 TVminus");
    SPG_CHECK_ARG(loss_out && workspace && (E == 0 || (is_transition && weights && diff && dl)), "bad argument");
    Carve w(workspace, workspace_bytes);
    partials = EdgeForwardWs(w, E).partials;
    SPG_CHECK_ARG(w.ok, "workspace too small (spg_edge_forward_workspace_bytes)");
  }
  hipStream_t st = (hipStream_t)stream;
  FwdArgs a{};
  a.emb = emb; a.ends = (const int2*)ends; a.trans = is_transition; a.weights = weights; a.diff = diff;
  a.dx = dist_type == DIST_INTRINSIC ? dx : nullptr;
  a.dl = dl; a.partials = partials; a.E = E; a.d = d; a.dist_type = dist_type; a.intra = intra; a.inter = inter;
  const int nb = spg_cdiv(E, EL_BLOCK);
  if (nb > 0) {
#define EL_FWD(DT)                                                                                                 \
  do {                                                                                                             \
    if (do_loss) hipLaunchKernelGGL((edge_fwd_kernel<true, true, DT>), dim3(nb), dim3(EL_BLOCK), 0, st, a);        \
    else hipLaunchKernelGGL((edge_fwd_kernel<true, false, DT>), dim3(nb), dim3(EL_BLOCK), 0, st, a);               \
  } while (0)
    if (!do_dist) hipLaunchKernelGGL((edge_fwd_kernel<false, true, 0>), dim3(nb), dim3(EL_BLOCK), 0, st, a);
    else if (dist_type == DIST_EUCLIDIAN) EL_FWD(DIST_EUCLIDIAN);
    else if (dist_type == DIST_INTRINSIC) EL_FWD(DIST_INTRINSIC);
    else EL_FWD(DIST_SCALAR);
#undef EL_FWD
    SPG_LAUNCH_CHECK();
  }
  if (do_loss) {
    hipLaunchKernelGGL(edge_loss_final_kernel, dim3(1), dim3(EL_BLOCK), 0, st, (const double*)partials, (long)nb, loss_out);
    SPG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int spg_edge_loss_backward(const float* dl, const uint8_t* is_transition, const float* up, long E, float* grad_diff, void* stream) {
  SPG_CHECK_ARG(E >= 0 && E < INT_MAX / 2 && up && (E == 0 || (dl && is_transition && grad_diff)), "bad argument");
  if (E == 0) return 0;
  hipLaunchKernelGGL(edge_loss_bwd_kernel, dim3(spg_cdiv(E, EL_BLOCK)), dim3(EL_BLOCK), 0, (hipStream_t)stream, dl, is_transition, up, E, grad_diff);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_edge_backward(const float* emb, long n, int d, const int32_t* rowptr, const uint32_t* inc, const int32_t* ends, long E,
                                 int dist_type, const float* dl, const uint8_t* is_transition, const float* up, const float* grad_diff,
                                 const float* dx, float* grad_emb, void* stream) {
  SPG_CHECK_ARG(sizes_ok(n, E), "1 <= n < 2^31 - 1 and 0 <= E < 2^30");
  SPG_CHECK_ARG(d >= 1 && d <= 64, "1 <= d <= 64");
  SPG_CHECK_ARG(dist_type >= DIST_EUCLIDIAN && dist_type <= DIST_SCALAR, "dist_type: 0 euclidian, 1 intrinsic, 2 scalar");
  SPG_CHECK_ARG(emb && rowptr && grad_emb && (E == 0 || (inc && ends)), "bad argument");
  SPG_CHECK_ARG(E == 0 || dl || grad_diff, "dl (with is_transition and up) or grad_diff");
  SPG_CHECK_ARG(!dl || (is_transition && up), "dl needs is_transition and up");
  SPG_CHECK_ARG(dist_type != DIST_INTRINSIC || E == 0 || dx, "intrinsic needs dx");
  BwdArgs a{};
  a.emb = emb; a.rowptr = rowptr; a.inc = inc; a.ends = (const int2*)ends; a.dl = dl; a.trans = is_transition; a.up = up;
  a.gdiff = grad_diff; a.dx = dist_type == DIST_INTRINSIC ? dx : nullptr; a.grad = grad_emb; a.n = n; a.d = d;
  a.euclid = dist_type == DIST_EUCLIDIAN;
  hipStream_t st = (hipStream_t)stream;
  if (d <= 1) launch_bwd<1>(a, st);
  else if (d <= 2) launch_bwd<2>(a, st);
  else if (d <= 4) launch_bwd<4>(a, st);
  else if (d <= 8) launch_bwd<8>(a, st);
  else if (d <= 16) launch_bwd<16>(a, st);
  else if (d <= 32) launch_bwd<32>(a, st);
  else launch_bwd<64>(a, st);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spg_cc_workspace_bytes(long n) {
  Carve w;
  CcWs l(w, std::max<long>(n, 1));
  return w.used();
}

extern "C" int spg_connected_components(const int32_t* ends, const uint8_t* active, long E, long n, int32_t* in_component,
                                        int32_t* component_size, int32_t* n_components, void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(sizes_ok(n, E), "1 <= n < 2^31 - 1 and 0 <= E < 2^30");
  SPG_CHECK_ARG(in_component && component_size && n_components && workspace && (E == 0 || (ends && active)), "bad argument");
  Carve w(workspace, workspace_bytes);
  CcWs l(w, n);
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_cc_workspace_bytes)");
  return cc_run((const int2*)ends, active, E, n, in_component, component_size, n_components, l, (hipStream_t)stream);
}

extern "C" size_t spg_xpart_workspace_bytes(long n, long E) {
  Carve w;
  XpartWs l(w, std::max<long>(n, 1), std::max<long>(E, 1));
  return w.used();
}

extern "C" int spg_xpart_weights(const int32_t* ends, long E, long n, const int32_t* pred_in_component, const uint8_t* is_transition,
                                 double factor, float* weights, int32_t* in_component, int32_t* component_size, int32_t* n_components,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(sizes_ok(n, E), "1 <= n < 2^31 - 1 and 0 <= E < 2^30");
  SPG_CHECK_ARG(pred_in_component && in_component && component_size && n_components && workspace && (E == 0 || (ends && is_transition && weights)),
                "bad argument");
  hipStream_t st = (hipStream_t)stream;
  Carve w(workspace, workspace_bytes);
  XpartWs l(w, n, std::max<long>(E, 1));
  uint8_t* active = l.active;
  u64 *k0 = l.k0, *k1 = l.k1, *ukeys = l.ukeys;
  unsigned *counts = l.counts, *nruns = l.nruns;
  void* tmp = l.tmp;
  const size_t tmp_bytes = l.tmp_bytes;
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_xpart_workspace_bytes)");
  const dim3 block(EL_BLOCK), ge(spg_cdiv(std::max<long>(E, 1), EL_BLOCK));
  if (E > 0) {
    hipLaunchKernelGGL(xp_active_kernel, ge, block, 0, st, (const int2*)ends, pred_in_component, is_transition, E, active);
    SPG_LAUNCH_CHECK();
  }
  SPG_TRY(cc_run((const int2*)ends, active, E, n, in_component, component_size, n_components, l.cc, st));
  if (E == 0) return 0;
  hipLaunchKernelGGL(xp_keys_kernel, ge, block, 0, st, (const int2*)ends, (const int32_t*)in_component, is_transition, E, k0);
  SPG_LAUNCH_CHECK();
  size_t b = tmp_bytes;
  SPG_RP(rocprim::radix_sort_keys(tmp, b, (const u64*)k0, k1, (size_t)E, 0, 64, st));
  b = tmp_bytes;
  SPG_RP(rocprim::run_length_encode(tmp, b, (const u64*)k1, (unsigned)E, ukeys, counts, nruns, st));
  hipLaunchKernelGGL(xp_weights_kernel, ge, block, 0, st, (const int2*)ends, (const int32_t*)in_component, (const int32_t*)component_size,
                     is_transition, E, (const u64*)ukeys, (const unsigned*)counts, (const unsigned*)nruns, factor, weights);
  SPG_LAUNCH_CHECK();
  return 0;
}
