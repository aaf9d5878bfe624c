// Neighbourhood sub-sampling of a resident superpoint graph (reference learning/spg.py:115-144: permute_vertices ->
// random_neighborhoods -> k_big_enough), restated in ORIGINAL vertex ids: the scene's graph stays in device
// memory, the host draws the permutation and the centres, and a sample -- its vertices, relabelled edges, edge-feature rows and
// in-degrees -- is cut out of it here.
//
//   inverse     inv[perm[k]] = k (ss_inverse_kernel), then perm[inv[j]] == j for every j (ss_check_kernel): an entry outside
//               [0, n) or a repeated one sets bit 1 of the error word.  inv is zeroed first, so every entry is a valid index.
//   levels      level[v] = 0 for v = inv[centre] (ss_centres_kernel; a centre outside [0, n) sets bit 0 and is left out), else -1;
//               without centres every vertex is on level 0.  Level L = 1 ... min(order, n - 1), one launch each
//               (ss_level_kernel, one lane per edge): a lane that sees one end on level L - 1 and the other end unmarked stores L
//               there.  Concurrent stores write the same value and a lane that reads a vertex while another marks it sees -1 or
//               L, never L - 1: the members are the same from run to run.  A search that has run out of vertices marks nothing.
//   cut         ONE exclusive scan (rocPRIM) over the permuted positions j of the pair (member and big, member) packed into 64
//               bits, v = inv[j], big = sizes[v] >= minpts.  Position j is kept iff it is a member and the inclusive count of
//               big ones is <= hardcutoff; every member in front of a kept position is kept too, so the exclusive member count IS
//               the new id (ss_vertices_kernel: vids, new_id, m by atomicMax).
//   edges       exclusive scan of "both ends kept" over the edges in file order, then ss_edges_kernel (kept edge id, relabelled
//               ends, atomicAdd on the target's in-degree: integers, the order does not matter) and ss_feats_kernel (one lane
//               per element of a feature row: a plain copy).
// Every loop is bounded by n, E or order; no kernel waits on another workgroup.
#include <climits>
#include <cstring>

#include "../../include/spg_hip.h"
#include "spg_part.h"

namespace {

constexpr int SS_BLOCK = 256;

struct CutArgs {
  const int* inv;          // null: the identity
  const int* level;
  const int64_t* sizes;    // null without a cut
  long minpts;
  int cut;                 // hardcutoff > 0
};

__device__ __forceinline__ int position_vertex(const CutArgs& a, int j) { return a.inv != nullptr ? a.inv[j] : j; }

// (member and big) << 32 | member of permuted position j
struct CutFlags {
  CutArgs a;
  __device__ u64 operator()(int j) const {
    const int v = position_vertex(a, j);
    if (a.level[v] < 0) return 0ull;
    const u64 big = (a.cut && a.sizes[v] >= a.minpts) ? 1ull : 0ull;
    return (big << 32) | 1ull;
  }
};

struct EdgeKept {
  const int2* ends;
  const int* new_id;
  __device__ int operator()(int e) const {
    const int2 en = ends[e];
    return (new_id[en.x] >= 0 && new_id[en.y] >= 0) ? 1 : 0;
  }
};

typedef rocprim::counting_iterator<int> Counting;

struct SampleWs {      // inverse permutation, level, new id per vertex; both prefix sums; rocPRIM scratch
  int *inv, *level, *new_id, *pe;
  u64* pv;
  void* tmp; size_t tmp_bytes;
  SampleWs(Carve& w, long n, long E) {
    inv = w.take_n<int>(n); level = w.take_n<int>(n); new_id = w.take_n<int>(n);
    pv = w.take_n<u64>(n);
    pe = w.take_n<int>(E);
    tmp_bytes = std::max(exclusive_scan_bytes<u64>(n, rocprim::make_transform_iterator(Counting(0), CutFlags())),
                         exclusive_scan_bytes<int>(E, rocprim::make_transform_iterator(Counting(0), EdgeKept())));
    tmp = w.take(tmp_bytes);
  }
};

__global__ __launch_bounds__(SS_BLOCK) void ss_inverse_kernel(const int64_t* __restrict__ perm, long n, int* __restrict__ inv,
                                                              u64* __restrict__ head) {
  const long k = (long)blockIdx.x * SS_BLOCK + threadIdx.x;
  if (k >= n) return;
  const int64_t p = perm[k];
  if (p < 0 || p >= n) { atomicOr(&head[2], 2ull); return; }
  inv[p] = (int)k;
}

__global__ __launch_bounds__(SS_BLOCK) void ss_check_kernel(const int64_t* __restrict__ perm, long n, const int* __restrict__ inv,
                                                            u64* __restrict__ head) {
  const long j = (long)blockIdx.x * SS_BLOCK + threadIdx.x;
  if (j >= n) return;
  if (perm[inv[j]] != j) atomicOr(&head[2], 2ull);
}

__global__ __launch_bounds__(SS_BLOCK) void ss_centres_kernel(const int64_t* __restrict__ centres, long n_centres, long n,
                                                              const int* __restrict__ inv, int* __restrict__ level, u64* __restrict__ head) {
  const long i = (long)blockIdx.x * SS_BLOCK + threadIdx.x;
  if (i >= n_centres) return;
  const int64_t c = centres[i];
  if (c < 0 || c >= n) { atomicOr(&head[2], 1ull); return; }
  level[inv != nullptr ? inv[c] : (int)c] = 0;
}

__global__ __launch_bounds__(SS_BLOCK) void ss_level_kernel(const int2* __restrict__ ends, long E, int L, int* level) {
  const long e = (long)blockIdx.x * SS_BLOCK + threadIdx.x;
  if (e >= E) return;
  const int2 en = ends[e];
  const int la = level[en.x], lb = level[en.y];
  if (la == L - 1 && lb < 0) level[en.y] = L;
  if (lb == L - 1 && la < 0) level[en.x] = L;
}

__global__ __launch_bounds__(SS_BLOCK) void ss_vertices_kernel(CutArgs a, const u64* __restrict__ pv, long n, long hardcutoff,
                                                               int64_t* __restrict__ vids, int* __restrict__ new_id,
                                                               u64* __restrict__ head) {
  const long j = (long)blockIdx.x * SS_BLOCK + threadIdx.x;
  if (j >= n) return;
  const int v = position_vertex(a, (int)j);
  const u64 own = CutFlags{a}((int)j), before = pv[j];
  const long big = (long)((before + own) >> 32), rank = (long)(before & 0xffffffffull);
  const bool kept = (own & 1ull) != 0 && (!a.cut || big <= hardcutoff);
  new_id[v] = kept ? (int)rank : -1;
  if (kept) {
    vids[rank] = v;
    atomicMax(&head[0], (u64)(rank + 1));
  }
}

__global__ __launch_bounds__(SS_BLOCK) void ss_edges_kernel(const int2* __restrict__ ends, long E, const int* __restrict__ new_id,
                                                            const int* __restrict__ pe, int64_t* __restrict__ edges_out,
                                                            int64_t* __restrict__ kept, u64* __restrict__ degs, u64* __restrict__ head) {
  const long e = (long)blockIdx.x * SS_BLOCK + threadIdx.x;
  if (e >= E) return;
  const int2 en = ends[e];
  const int a = new_id[en.x], b = new_id[en.y], p = pe[e];
  const bool k = a >= 0 && b >= 0;
  if (k) {
    kept[p] = e;
    edges_out[2 * (long)p] = a; edges_out[2 * (long)p + 1] = b;
    atomicAdd(&degs[b], 1ull);
  }
  if (e == E - 1) head[1] = (u64)(p + (k ? 1 : 0));
}

__global__ __launch_bounds__(SS_BLOCK) void ss_feats_kernel(const int2* __restrict__ ends, long E, int F, const int* __restrict__ new_id,
                                                            const int* __restrict__ pe, const float* __restrict__ feats,
                                                            float* __restrict__ feats_out) {
  const long t = (long)blockIdx.x * SS_BLOCK + threadIdx.x;
  if (t >= E * F) return;
  const long e = t / F;
  const int c = (int)(t - e * F);
  const int2 en = ends[e];
  if (new_id[en.x] >= 0 && new_id[en.y] >= 0) feats_out[(long)pe[e] * F + c] = feats[t];
}

}  // namespace

extern "C" size_t spg_sample_spg_workspace_bytes(long n, long E) {
  Carve w;
  SampleWs l(w, std::max<long>(n, 1), std::max<long>(E, 1));
  return w.used();
}

extern "C" int spg_sample_spg(const int32_t* ends, long E, long n, const int64_t* perm, const int64_t* centres, long n_centres,
                              const int64_t* sizes, const float* feats, int F, int order, long minpts, long hardcutoff, int64_t* vids,
                              int64_t* edges_out, int64_t* kept, float* feats_out, int64_t* degs, int64_t* head, void* workspace,
                              size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(n >= 1 && n < INT_MAX && E >= 0 && E < INT_MAX / 2, "1 <= n < 2^31 - 1 and 0 <= E < 2^30");
  SPG_CHECK_ARG(order >= 0 && n_centres >= 0 && n_centres < INT_MAX && (centres != nullptr || n_centres == 0), "bad order or centres");
  SPG_CHECK_ARG(hardcutoff <= 0 || sizes != nullptr, "a cut (hardcutoff > 0) needs sizes");
  SPG_CHECK_ARG(F >= 0 && F < 4096 && (feats == nullptr) == (feats_out == nullptr), "feats and feats_out come together, 0 <= F < 4096");
  SPG_CHECK_ARG(E * std::max(F, 1) < (1l << 38), "E * F < 2^38");
  SPG_CHECK_ARG(vids && degs && head && workspace && (E == 0 || (ends && edges_out && kept)), "bad argument");
  hipStream_t st = (hipStream_t)stream;
  Carve w(workspace, workspace_bytes);
  SampleWs l(w, n, std::max<long>(E, 1));
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_sample_spg_workspace_bytes)");
  u64* hd = (u64*)head;
  const int2* en = (const int2*)ends;
  const dim3 block(SS_BLOCK), grid_n(spg_cdiv(n, SS_BLOCK)), grid_e(spg_cdiv(std::max<long>(E, 1), SS_BLOCK));
  SPG_RP(hipMemsetAsync(head, 0, 3 * sizeof(int64_t), st));
  SPG_RP(hipMemsetAsync(degs, 0, (size_t)n * sizeof(int64_t), st));
  const int* inv = nullptr;
  if (perm != nullptr) {
    SPG_RP(hipMemsetAsync(l.inv, 0, (size_t)n * sizeof(int), st));
    hipLaunchKernelGGL(ss_inverse_kernel, grid_n, block, 0, st, perm, n, l.inv, hd);
    SPG_LAUNCH_CHECK();
    hipLaunchKernelGGL(ss_check_kernel, grid_n, block, 0, st, perm, n, (const int*)l.inv, hd);
    SPG_LAUNCH_CHECK();
    inv = l.inv;
  }
  // members: level >= 0
  SPG_RP(hipMemsetAsync(l.level, centres != nullptr ? 0xFF : 0, (size_t)n * sizeof(int), st));
  if (centres != nullptr) {
    if (n_centres > 0) {
      hipLaunchKernelGGL(ss_centres_kernel, dim3(spg_cdiv(n_centres, SS_BLOCK)), block, 0, st, centres, n_centres, n, inv, l.level, hd);
      SPG_LAUNCH_CHECK();
    }
    const long levels = E > 0 ? std::min<long>(order, n - 1) : 0;
    for (long L = 1; L <= levels; ++L) {
      hipLaunchKernelGGL(ss_level_kernel, grid_e, block, 0, st, en, E, (int)L, l.level);
      SPG_LAUNCH_CHECK();
    }
  }
  // the cut and the new ids
  CutArgs a;
  a.inv = inv; a.level = l.level; a.sizes = sizes; a.minpts = minpts; a.cut = hardcutoff > 0 ? 1 : 0;
  size_t b = l.tmp_bytes;
  SPG_RP(rocprim::exclusive_scan(l.tmp, b, rocprim::make_transform_iterator(Counting(0), CutFlags{a}), l.pv, (u64)0, (size_t)n,
                                 rocprim::plus<u64>(), st));
  hipLaunchKernelGGL(ss_vertices_kernel, grid_n, block, 0, st, a, (const u64*)l.pv, n, hardcutoff, vids, l.new_id, hd);
  SPG_LAUNCH_CHECK();
  if (E == 0) return 0;
  b = l.tmp_bytes;
  SPG_RP(rocprim::exclusive_scan(l.tmp, b, rocprim::make_transform_iterator(Counting(0), EdgeKept{en, l.new_id}), l.pe, 0, (size_t)E,
                                 rocprim::plus<int>(), st));
  hipLaunchKernelGGL(ss_edges_kernel, grid_e, block, 0, st, en, E, (const int*)l.new_id, (const int*)l.pe, edges_out, kept, (u64*)degs, hd);
  SPG_LAUNCH_CHECK();
  if (feats != nullptr && F > 0) {
    hipLaunchKernelGGL(ss_feats_kernel, dim3(spg_cdiv(E * F, SS_BLOCK)), block, 0, st, en, E, F, (const int*)l.new_id, (const int*)l.pe, feats,
                       feats_out);
    SPG_LAUNCH_CHECK();
  }
  return 0;
}
