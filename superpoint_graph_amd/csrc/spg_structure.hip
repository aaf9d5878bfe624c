// The scene structure of the learned partition made on the device: the glue arithmetic of the per-file body of the reference's
// supervized_partition/graph_processing.py:main() (:126, :144-190) between the steps that already have kernels (prune, kNN,
// connected components, compute_geof).  Three entry points, all streaming and memory-bound: every global access is coalesced
// (consecutive lanes, consecutive addresses) and nothing is read twice.
//
// Frame (spg_structure_frame): min z, min x, min y, max x, max y of xyz [n, 3] by the two-phase pass of spg_part.h (FramePass).  Min
//   and max do not depend on the order, so the values are those of np.min / np.max (up to the sign of a zero, which numpy leaves
//   open too).  A coordinate that is not finite sets bit 0 of the error word.
// Vertices (spg_structure_vertices): vertices_kernel, 256 vertices per workgroup.
//   values   one lane per vertex: elevation = z - min z; xyn = (xy - mi) / ((ma - mi) + 1e-8f), every step rounded to float32
//            on its own and ONE correctly rounded division (numpy keeps float32 when a float32 array meets a Python scalar);
//            rgb / 255 (graph_processing.py:353) the same way; geof[:, 3] doubled in place (:177, exact).
//   ids      the hard id of a histogram row: G lanes per row (G a power of two >= the columns, at most 64) read consecutive
//            columns, keep (largest count, smallest column) and combine by xor shuffles inside their group -- np.argmax's first
//            maximum.  The column range starts at 1 for the s3dis objects (`objects[:, 1:].argmax(1) + 1` IS the column) and at 0
//            for the vkitti labels; an all-zero row gives the first column of the range.  The 256 ids of the workgroup go through
//            LDS and are stored as one contiguous run.  Or the pass-through of an id vector (int32 / int64 -> int64).
// Edges (spg_structure_edges): edges_kernel, one lane per entry (vertex, column) of the kNN table [n, k_local]: every index is
//   checked against [0, n) (bit 1 of the error word; read as 0), the first k_adj columns are the adjacency: edg_source =
//   repeat(arange(n), k_adj), edg_target, is_transition = id[source] != id[target] and its complement.
// No contraction (#pragma clang fp contract(off)), no atomics on floats, no inter-workgroup waiting.
#include <climits>
#include <cstring>

#include "../../include/spg_hip.h"
#include "spg_part.h"

namespace {

constexpr int ST_BLOCK = PART_BLOCK;

// ---- frame -------------------------------------------------------------------------------------------------------------
// the pass (spg_part.h) of the minima (z, x, y), the maxima (x, y) and the finite check -> frame [5]
struct FramePass {
  typedef float T;
  static constexpr int K = 5;
  static constexpr int op(int c) { return c < 3 ? PART_MIN : PART_MAX; }
  float* frame;
  __device__ void point(const float* __restrict__ xyz, long i, float (&v)[5], int& bad) const {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    bad |= !(finite_f32(x) && finite_f32(y) && finite_f32(z));
    v[0] = fminf(v[0], z); v[1] = fminf(v[1], x); v[2] = fminf(v[2], y);
    v[3] = fmaxf(v[3], x); v[4] = fmaxf(v[4], y);
  }
  __device__ void write(const float (&v)[5], long) const {
#pragma unroll
    for (int c = 0; c < 5; ++c) frame[c] = v[c];
  }
};

// ---- vertices ----------------------------------------------------------------------------------------------------------
struct VertexArgs {
  const float* xyz;          // [n, 3]
  const float* frame;        // [5]: min z, min x, min y, max x, max y
  const uint8_t* rgb_u8;     // [n, 3] or null
  const uint32_t* hist;      // [n, C] or null
  const void* ids_in;        // [n] int32 / int64 or null
  float* elevation;          // [n] or null
  float* xyn;                // [n, 2] or null
  float* rgb;                // [n, 3] (with rgb_u8)
  float* geof;               // [n, 4] or null: column 3 doubled in place
  int64_t* hard_ids;         // [n] (with hist or ids_in)
  long n;
  int C, first_col, G, ids_is_i64;
};

__global__ __launch_bounds__(ST_BLOCK) void vertices_kernel(VertexArgs a) {
#pragma clang fp contract(off)
  __shared__ int ids[ST_BLOCK];
  const long base = (long)blockIdx.x * ST_BLOCK;
  const long v = base + threadIdx.x;
  if (v < a.n) {
    const float x = a.xyz[3 * v], y = a.xyz[3 * v + 1], z = a.xyz[3 * v + 2];
    if (a.elevation) a.elevation[v] = z - a.frame[0];
    if (a.xyn) {
      const float mix = a.frame[1], miy = a.frame[2];
      const float ex = a.frame[3] - mix, ey = a.frame[4] - miy;        // ma - mi, rounded
      const float dx = ex + 1e-8f, dy = ey + 1e-8f;                    // + float32(1e-8), rounded
      float2 o;
      o.x = __fdiv_rn(x - mix, dx);
      o.y = __fdiv_rn(y - miy, dy);
      reinterpret_cast<float2*>(a.xyn)[v] = o;
    }
    if (a.geof) a.geof[4 * v + 3] = 2.f * a.geof[4 * v + 3];
    if (a.ids_in) a.hard_ids[v] = a.ids_is_i64 ? ((const int64_t*)a.ids_in)[v] : (int64_t)((const int32_t*)a.ids_in)[v];
  }
  if (a.rgb_u8) {      // the [256, 3] block of the workgroup is one contiguous range: consecutive lanes, consecutive bytes
    const long end = 3 * a.n;
    for (long i = 3 * base + threadIdx.x; i < 3 * (base + ST_BLOCK) && i < end; i += ST_BLOCK) a.rgb[i] = __fdiv_rn((float)a.rgb_u8[i], 255.f);
  }
  if (a.hist) {
    const int G = a.G, sub = threadIdx.x & (G - 1), rows_per_pass = ST_BLOCK / G;
    for (int r = threadIdx.x / G; r < ST_BLOCK; r += rows_per_pass) {      // the same trip count in every lane
      const long row = base + r;
      unsigned best_v = 0;
      int best_c = INT_MAX;
      if (row < a.n) {
        const uint32_t* h = a.hist + row * a.C;
        for (int c = a.first_col + sub; c < a.C; c += G) {
          const unsigned hv = h[c];
          if (hv > best_v || (hv == best_v && c < best_c)) { best_v = hv; best_c = c; }
        }
      }
      for (int off = G >> 1; off >= 1; off >>= 1) {                          // (xor below G stays inside the group)
        const unsigned ov = __shfl_xor(best_v, off, 64);
        const int oc = __shfl_xor(best_c, off, 64);
        if (ov > best_v || (ov == best_v && oc < best_c)) { best_v = ov; best_c = oc; }
      }
      if (sub == 0) ids[r] = best_c;
    }
    __syncthreads();
    if (v < a.n) a.hard_ids[v] = ids[threadIdx.x];
  }
}

// ---- edges -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_BLOCK) void edges_kernel(const int32_t* __restrict__ idx, long n, int k_local, int k_adj,
                                                         const int64_t* __restrict__ ids, int64_t* __restrict__ edg_source,
                                                         int64_t* __restrict__ edg_target, uint8_t* __restrict__ is_transition,
                                                         uint8_t* __restrict__ active, int32_t* __restrict__ err) {
  const long i = (long)blockIdx.x * ST_BLOCK + threadIdx.x;
  int bad = 0;
  if (i < n * k_local) {
    const long v = i / k_local;
    const int j = (int)(i - v * k_local);
    long t = idx[i];
    if (t < 0 || t >= n) { bad = 1; t = 0; }
    if (j < k_adj) {
      const long e = v * k_adj + j;
      edg_source[e] = v;
      edg_target[e] = t;
      if (ids) {
        const uint8_t tr = ids[v] != ids[t];
        is_transition[e] = tr;
        active[e] = !tr;
      }
    }
  }
  block_report(bad, err, 2);
}

struct FrameWs {
  float* partials;           // [blocks, 5]
  int blocks;
  FrameWs(Carve& w, long n) {
    blocks = part_reduce_blocks(n);
    partials = w.take_n<float>((size_t)blocks * 5);
  }
};

}  // namespace

extern "C" size_t spg_structure_frame_workspace_bytes(long n) {
  Carve w;
  FrameWs l(w, n);
  return w.used();
}

extern "C" int spg_structure_frame(const float* xyz, long n, float* frame, int32_t* error_flag, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  SPG_CHECK_ARG(xyz && frame && error_flag && workspace, "bad argument");
  SPG_CHECK_ARG(n >= 1 && n < INT_MAX, "1 <= n < 2^31 - 1");
  Carve w(workspace, workspace_bytes);
  FrameWs l(w, n);
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_structure_frame_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  SPG_RP(hipMemsetAsync(error_flag, 0, sizeof(int32_t), st));
  if (int rc = part_reduce(FramePass{frame}, xyz, n, l.partials, l.blocks, error_flag, st)) return rc;
  return 0;
}

extern "C" int spg_structure_vertices(const float* xyz, long n, const float* frame, const uint8_t* rgb_u8, const void* hist, int hist_cols,
                                      int id_mode, const void* ids_in, int ids_is_i64, float* elevation, float* xyn, float* rgb, float* geof,
                                      int64_t* hard_ids, void* stream) {
  SPG_CHECK_ARG(xyz && frame, "bad argument");
  SPG_CHECK_ARG(n >= 1 && n < INT_MAX, "1 <= n < 2^31 - 1");
  SPG_CHECK_ARG(id_mode >= SPG_STRUCTURE_IDS_NONE && id_mode <= SPG_STRUCTURE_IDS_GIVEN, "id_mode: 0 none, 1 objects, 2 labels, 3 given");
  SPG_CHECK_ARG((rgb_u8 == nullptr) == (rgb == nullptr), "rgb_u8 and rgb go together");
  SPG_CHECK_ARG(xyn == nullptr || (((uintptr_t)xyn) & 7) == 0, "xyn must be 8-byte aligned");
  VertexArgs a{};
  a.xyz = xyz; a.frame = frame; a.rgb_u8 = rgb_u8; a.elevation = elevation; a.xyn = xyn; a.rgb = rgb; a.geof = geof; a.n = n;
  a.G = 1;
  if (id_mode == SPG_STRUCTURE_IDS_OBJECTS || id_mode == SPG_STRUCTURE_IDS_LABELS) {
    a.first_col = id_mode == SPG_STRUCTURE_IDS_OBJECTS ? 1 : 0;
    SPG_CHECK_ARG(hist && hard_ids, "a histogram id needs hist and hard_ids");
    SPG_CHECK_ARG(hist_cols > a.first_col && (long)hist_cols * n < (1l << 40), "the histogram has no column to take the arg-max over");
    a.hist = (const uint32_t*)hist; a.C = hist_cols; a.hard_ids = hard_ids;
    while (a.G < 64 && a.G < hist_cols) a.G <<= 1;
  } else if (id_mode == SPG_STRUCTURE_IDS_GIVEN) {
    SPG_CHECK_ARG(ids_in && hard_ids && ids_in != (const void*)hard_ids, "a given id needs ids_in and a distinct hard_ids");
    a.ids_in = ids_in; a.ids_is_i64 = ids_is_i64; a.hard_ids = hard_ids;
  }
  hipLaunchKernelGGL(vertices_kernel, dim3(spg_cdiv(n, ST_BLOCK)), dim3(ST_BLOCK), 0, (hipStream_t)stream, a);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_structure_edges(const int32_t* knn_idx, long n, int k_local, int k_adj, const int64_t* hard_ids, int64_t* edg_source,
                                   int64_t* edg_target, uint8_t* is_transition, uint8_t* active, int32_t* error_flag, void* stream) {
  SPG_CHECK_ARG(knn_idx && edg_source && edg_target && error_flag, "bad argument");
  SPG_CHECK_ARG(n >= 1 && n < INT_MAX && k_local >= 1 && k_adj >= 1 && k_adj <= k_local, "1 <= n < 2^31 - 1, 1 <= k_adj <= k_local");
  SPG_CHECK_ARG(n * k_adj < INT_MAX / 2 && n * k_local < (long)INT_MAX * ST_BLOCK, "n * k_adj < 2^30 edges");
  SPG_CHECK_ARG(hard_ids == nullptr || (is_transition && active), "hard_ids need is_transition and active");
  hipLaunchKernelGGL(edges_kernel, dim3(spg_cdiv(n * k_local, ST_BLOCK)), dim3(ST_BLOCK), 0, (hipStream_t)stream, knn_idx, n, k_local, k_adj,
                     hard_ids, edg_source, edg_target, is_transition, active, error_flag);
  SPG_LAUNCH_CHECK();
  return 0;
}
