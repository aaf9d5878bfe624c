// Batches of the learned (supervised) partition made on the device (reference supervized_partition/graph_processing.py:347-436
// graph_loader, :534-546 augment_cloud_whole, partition/ply_c/random_subgraph.cpp): the scene stays in device memory and a
// batch -- the k-nearest-neighbour tiles, their global features, the sampled subgraph and its relabelled edges -- is built there.
//
// Neighbourhood tiles (spg_neighbourhood_tiles): tiles_kernel, TL_VPB = 32 selected vertices per workgroup of 256 lanes.
//   gather   lane = (vertex, neighbour): nei[row, j], the neighbour's xyz (and rgb) into LDS as [vertex][channel][j] -- the layout
//            of the output block, so that every neighbour is fetched once;
//   stats    one lane per (vertex, axis): sum over j = 0 ... k - 1 in order, / k, squared deviations in the same order, / k --
//            the float32 sequence numpy runs for clouds.var(1) (a reduction over a non-contiguous axis adds row after row);
//   diam     one lane per vertex: sqrt((v0 + v1) + v2) correctly rounded, denominator diam + 1e-10f IN FLOAT32, the row of
//            clouds_global;
//   write    the [32, F, k] block of the workgroup is ONE contiguous range of clouds: consecutive lanes write consecutive
//            16-byte pieces (coordinates: (x - centre) / denominator, correctly rounded; colours: as staged).
//   The kernel writes F * k * 4 bytes per vertex (480 at F = 6, k = 20) against (8 + 12 or 24) * k gathered: write-bound.
//   No contraction anywhere (#pragma clang fp contract(off)): every product, sum and quotient is rounded on its own.
//   An index outside [0, N) in nei or rows sets the error word and is read as 0: nothing is read or written out of range.
// Whole-cloud augmentation (spg_augment_whole): one lane per coordinate: ((x - ref) @ M + ref) + noise, clip(rgb + noise, -1, 1).
// Random subgraph (spg_random_subgraph): rs_kernel, ONE workgroup, level-synchronous.  The reference's FIFO queue makes the
//   selection a breadth-first one whose order inside a level is (queue position of the parent, adjacency slot): every lane of
//   the frontier proposes its unselected neighbours with atomicMin of (position << 32 | slot) on a per-vertex key, the winners
//   are ranked by a workgroup scan (their rank is their position in the next frontier), and the first `size - count` of them
//   are accepted.  The level in which the count reaches the size ends the normal phase; what remains of the queue (the rest of
//   the frontier behind the parent of the last accepted vertex, then the vertices accepted in this level) examines its FIRST
//   adjacency slot only, and the first of those that is unselected is accepted as vertex size + 1 (random_subgraph.cpp:75,
//   `node_seen <= subgraph_size`).  Every loop is bounded by n; there is no waiting on other workgroups.
// Induced subgraph (spg_induced_subgraph): exclusive scans (rocPRIM) of both masks, then one launch over the vertices (rows,
//   new_ver_index) and one over the edges (kept edge ids, relabelled ends).
#include <climits>
#include <cstring>

#include "../../include/spg_hip.h"
#include "spg_part.h"

namespace {

constexpr int TL_BLOCK = 256;
constexpr int TL_VPB = 32;             // selected vertices per workgroup (include/spg_hip.h: SPG_TILES_VERTICES_PER_BLOCK)
constexpr int TL_MAX_K = 64;
constexpr int RS_BLOCK = 1024;
constexpr u64 RS_FREE = ~0ull;

static_assert(TL_VPB == SPG_TILES_VERTICES_PER_BLOCK, "header and kernel disagree");

// -------------------------------------------------------------------------------------------------------------------
// neighbourhood tiles
// -------------------------------------------------------------------------------------------------------------------
struct TileGlobals {
  const float* elevation;   // [N] or null
  const float* xyn;         // [N, 2] or null
  int own_rgb;              // the vertex's own rgb (needs rgb)
  int own_xy;               // xyz[row, :2]
  int G;                    // columns of clouds_global
};

template <typename IDX, bool STREAM>
__global__ __launch_bounds__(TL_BLOCK) void tiles_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb, int cloud_rgb,
                                                         const IDX* __restrict__ nei, long K, int k, const int64_t* __restrict__ rows,
                                                         long m, long N, TileGlobals g, float* __restrict__ clouds,
                                                         float* __restrict__ clouds_global, float* __restrict__ diameters,
                                                         int32_t* __restrict__ flag) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float tl_lds[];
  __shared__ long srow[TL_VPB];
  const int F = cloud_rgb ? 6 : 3;
  const int Fk = F * k;
  float* pts = tl_lds;                       // [TL_VPB][F][k]
  float* cen = pts + TL_VPB * Fk;            // [TL_VPB][3]
  float* var = cen + TL_VPB * 3;             // [TL_VPB][3]
  float* den = var + TL_VPB * 3;             // [TL_VPB]
  const int tid = threadIdx.x;
  const long v0 = (long)blockIdx.x * TL_VPB;
  const int nv = (int)(m - v0 < TL_VPB ? m - v0 : TL_VPB);
  bool bad = false;
  if (tid < nv) {
    long r = rows != nullptr ? (long)rows[v0 + tid] : v0 + tid;
    if (r < 0 || r >= N) { bad = true; r = 0; }
    srow[tid] = r;
  }
  __syncthreads();
  if (tid < nv * 3) cen[tid] = xyz[srow[tid / 3] * 3 + tid % 3];
  for (int p = tid; p < nv * k; p += TL_BLOCK) {
    const int vi = p / k, j = p - vi * k;
    long idx = (long)nei[srow[vi] * K + j];
    if (idx < 0 || idx >= N) { bad = true; idx = 0; }
    float* o = pts + vi * Fk + j;
    const float* x = xyz + idx * 3;
    o[0] = x[0]; o[k] = x[1]; o[2 * k] = x[2];
    if (cloud_rgb) {
      const float* c = rgb + idx * 3;
      o[3 * k] = c[0]; o[4 * k] = c[1]; o[5 * k] = c[2];
    }
  }
  if (bad) atomicOr(flag, 1);
  __syncthreads();
  if (tid < nv * 3) {
    const int vi = tid / 3, a = tid - vi * 3;
    const float* p = pts + vi * Fk + a * k;
    const float fk = (float)k;
    float s = p[0];
    for (int j = 1; j < k; ++j) s = s + p[j];
    const float mean = __fdiv_rn(s, fk);
    float d = p[0] - mean;
    float q = d * d;
    for (int j = 1; j < k; ++j) {
      d = p[j] - mean;
      const float dd = d * d;
      q = q + dd;
    }
    var[tid] = __fdiv_rn(q, fk);
  }
  __syncthreads();
  if (tid < nv) {
    const float v01 = var[tid * 3] + var[tid * 3 + 1];
    const float diam = sqrt_rn_f32(v01 + var[tid * 3 + 2]);
    den[tid] = diam + 1e-10f;
    diameters[v0 + tid] = diam;
    const long r = srow[tid];
    float* cg = clouds_global + (v0 + tid) * g.G;
    int c = 0;
    cg[c++] = diam;
    if (g.elevation != nullptr) cg[c++] = g.elevation[r];
    if (g.own_rgb) { cg[c++] = rgb[r * 3]; cg[c++] = rgb[r * 3 + 1]; cg[c++] = rgb[r * 3 + 2]; }
    if (g.xyn != nullptr) { cg[c++] = g.xyn[r * 2]; cg[c++] = g.xyn[r * 2 + 1]; }
    if (g.own_xy) { cg[c++] = cen[tid * 3]; cg[c++] = cen[tid * 3 + 1]; }
  }
  __syncthreads();
  // the block of this workgroup: floats [v0 * Fk, (v0 + nv) * Fk) of clouds; v0 * Fk is a multiple of 32: 16-byte pieces are aligned
  const int total = nv * Fk;
  float* out = clouds + v0 * Fk;
  auto value = [&](float x, int vi, int c) { return c < 3 ? __fdiv_rn(x - cen[vi * 3 + c], den[vi]) : x; };
  const int quads = total >> 2;
  for (int o4 = tid; o4 < quads; o4 += TL_BLOCK) {
    const unsigned o = 4u * (unsigned)o4;
    int vi = (int)(o / (unsigned)Fk);
    const unsigned rem = o - (unsigned)vi * (unsigned)Fk;
    int c = (int)(rem / (unsigned)k), j = (int)(rem - (unsigned)c * (unsigned)k);
    const f32x4 x = reinterpret_cast<const f32x4*>(pts)[o4];
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {                      // (a piece may cross a channel or a vertex)
      v[i] = value(x[i], vi, c);
      if (++j == k) { j = 0; if (++c == F) { c = 0; ++vi; } }
    }
    if (STREAM) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(out) + o4);
    else reinterpret_cast<f32x4*>(out)[o4] = v;
  }
  for (int o = 4 * quads + tid; o < total; o += TL_BLOCK) {
    const int vi = o / Fk, c = (o - vi * Fk) / k;
    out[o] = value(pts[o], vi, c);
  }
}

// -------------------------------------------------------------------------------------------------------------------
// whole-cloud augmentation
// -------------------------------------------------------------------------------------------------------------------
struct AugmentArgs {
  float M[9];       // row-major [3, 3]: out = (x - ref) @ M + ref
  float ref[3];
  int rotate;
};

__global__ void augment_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb, long N, AugmentArgs a,
                               const float* __restrict__ noise_xyz, const float* __restrict__ noise_rgb, float* __restrict__ xyz_out,
                               float* __restrict__ rgb_out) {
#pragma clang fp contract(off)
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * 3) return;
  const long i = e / 3;
  const int c = (int)(e - i * 3);
  float v = xyz[e];
  if (a.rotate) {
    const float d0 = xyz[i * 3] - a.ref[0], d1 = xyz[i * 3 + 1] - a.ref[1], d2 = xyz[i * 3 + 2] - a.ref[2];
    const float p0 = d0 * a.M[c], p1 = d1 * a.M[3 + c], p2 = d2 * a.M[6 + c];
    const float s01 = p0 + p1;
    const float s = s01 + p2;
    v = s + a.ref[c];
  }
  if (noise_xyz != nullptr) v = v + noise_xyz[e];
  xyz_out[e] = v;
  if (rgb_out != nullptr) {
    float r = rgb[e];
    if (noise_rgb != nullptr) {
      r = r + noise_rgb[e];
      r = fminf(fmaxf(r, -1.f), 1.f);
    }
    rgb_out[e] = r;
  }
}

// -------------------------------------------------------------------------------------------------------------------
// random subgraph
// -------------------------------------------------------------------------------------------------------------------
// values other lanes of the workgroup wrote in an earlier phase (behind __threadfence + __syncthreads): read and written past
// the vector L1 cache
__device__ __forceinline__ int rs_ld8(const uint8_t* p) { return (int)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rs_st8(uint8_t* p, uint8_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 rs_ld64(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rs_st64(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int rs_ld32(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rs_st32(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// exclusive scan of v over the workgroup -> the lane's prefix; *total = the sum (the same value in every lane)
__device__ __forceinline__ int rs_exscan(int v, int* total, int* s_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();                                   // (the previous scan's readers are done with s_wave)
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int pre = 0, tot = 0;
  for (int w = 0; w < RS_BLOCK / 64; ++w) {
    const int x = s_wave[w];
    if (w < wave) pre += x;
    tot += x;
  }
  *total = tot;
  return pre + inc - v;
}

// the vertex at the other end of incidence slot s (inc = edge << 1 | side; side 0: this vertex is the edge's source)
__device__ __forceinline__ int rs_neighbour(const uint32_t* __restrict__ inc, const int32_t* __restrict__ ends, int s) {
  const uint32_t x = inc[s];
  return ends[2 * (long)(x >> 1) + (1 - (int)(x & 1u))];
}

// state[0] = vertices selected so far (in / out), state[1] = seeds consumed by this call (out), state[2] = error word (out:
// 1 = a seed outside [0, n)).  selected [n] in / out; key [n] all RS_FREE on entry and on exit; fr0 / fr1 [n] scratch.
__global__ __launch_bounds__(RS_BLOCK) void rs_kernel(const int32_t* __restrict__ rowptr, const uint32_t* __restrict__ inc,
                                                      const int32_t* __restrict__ ends, int n, int size, const int64_t* __restrict__ seeds,
                                                      int n_seeds, uint8_t* selected, u64* key, int* fr0, int* fr1, int64_t* state) {
  __shared__ int s_wave[RS_BLOCK / 64];
  __shared__ int s_cutq;
  __shared__ u64 s_first;
  const int tid = threadIdx.x;
  int count = (int)state[0];           // every variable below is uniform: all lanes compute the same values
  int si = 0, err = 0;
  int* cur = fr0;
  int* nxt = fr1;
  while (count < size && si < n_seeds) {
    const long sd = (long)seeds[si];
    if (sd < 0 || sd >= n) { err = 1; break; }
    ++si;
    if (rs_ld8(selected + sd) != 0) continue;                 // an already selected seed is skipped, and consumed
    __syncthreads();                                         // (every lane has read selected[sd])
    if (tid == 0) { rs_st8(selected + sd, 1); rs_st32(cur, (int)sd); }
    ++count;
    int F = 1, tail_from = 0, n_acc = 0;
    bool cut = count == size;                                // the seed itself completes the selection: it examines its first slot
    __threadfence();
    __syncthreads();
    for (int level = 0; !cut && F > 0 && level < n; ++level) {
      // proposals: the smallest (queue position, slot) that reaches an unselected vertex owns it
      for (int q = tid; q < F; q += RS_BLOCK) {
        const int v = rs_ld32(cur + q), b = rowptr[v], e = rowptr[v + 1];
        for (int s = b; s < e; ++s) {
          const int w = rs_neighbour(inc, ends, s);
          if (rs_ld8(selected + w) == 0) atomicMin(key + w, ((u64)(unsigned)q << 32) | (u64)(unsigned)(s - b));
        }
      }
      if (tid == 0) s_cutq = INT_MAX;
      __threadfence();
      __syncthreads();
      // ranks: the winners in (queue position, slot) order are the next frontier
      const int need = size - count;
      int T = 0;
      for (int base = 0; base < F; base += RS_BLOCK) {
        const int q = base + tid;
        int c = 0, v = 0, b = 0, e = 0;
        if (q < F) {
          v = rs_ld32(cur + q); b = rowptr[v]; e = rowptr[v + 1];
          for (int s = b; s < e; ++s)
            c += rs_ld64(key + rs_neighbour(inc, ends, s)) == (((u64)(unsigned)q << 32) | (u64)(unsigned)(s - b)) ? 1 : 0;
        }
        int tot;
        int r = T + rs_exscan(c, &tot, s_wave);
        if (c > 0) {
          for (int s = b; s < e; ++s) {
            const int w = rs_neighbour(inc, ends, s);
            if (rs_ld64(key + w) == (((u64)(unsigned)q << 32) | (u64)(unsigned)(s - b))) {
              rs_st32(nxt + r, w);
              if (r == need - 1) s_cutq = q;                  // the parent of the vertex that completes the selection
              ++r;
            }
          }
        }
        T += tot;
      }
      __threadfence();
      __syncthreads();
      const int acc = T < need ? T : need;
      for (int r = tid; r < T; r += RS_BLOCK) {
        const int w = rs_ld32(nxt + r);
        rs_st64(key + w, RS_FREE);
        if (r < acc) rs_st8(selected + w, 1);
      }
      count += acc;
      const int cutq = s_cutq;
      __threadfence();
      __syncthreads();
      if (T >= need) { cut = true; tail_from = cutq + 1; n_acc = acc; break; }
      int* t = cur; cur = nxt; nxt = t;
      F = T;
    }
    if (cut) {
      // the queue that is left: cur[tail_from, F), then nxt[0, n_acc); each examines its first adjacency slot only
      if (tid == 0) s_first = RS_FREE;
      __syncthreads();
      const int rest = F - tail_from, L = rest + n_acc;
      for (int i = tid; i < L; i += RS_BLOCK) {
        const int v = i < rest ? rs_ld32(cur + tail_from + i) : rs_ld32(nxt + (i - rest));
        const int b = rowptr[v];
        if (rowptr[v + 1] > b) {
          const int w = rs_neighbour(inc, ends, b);
          if (rs_ld8(selected + w) == 0) atomicMin(&s_first, ((u64)(unsigned)i << 32) | (u64)(unsigned)w);
        }
      }
      __syncthreads();
      const u64 first = s_first;
      if (first != RS_FREE) {
        if (tid == 0) rs_st8(selected + (int)(first & 0xFFFFFFFFull), 1);
        ++count;
      }
      __threadfence();
      __syncthreads();
      break;
    }
  }
  if (tid == 0) { state[0] = count; state[1] = si; state[2] = err; }
}

__global__ void rs_edges_kernel(const int2* __restrict__ ends, const uint8_t* __restrict__ selected, long E, uint8_t* __restrict__ selected_edg) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int2 en = ends[e];
  selected_edg[e] = (uint8_t)((selected[en.x] != 0 ? 1 : 0) * (selected[en.y] != 0 ? 1 : 0));
}

// -------------------------------------------------------------------------------------------------------------------
// induced subgraph
// -------------------------------------------------------------------------------------------------------------------
struct NonZero {
  __device__ int operator()(uint8_t x) const { return x != 0 ? 1 : 0; }
};

struct RandomSubgraphWs {      // per-vertex proposal keys, two frontiers
  u64* key;
  int *fr0, *fr1;
  RandomSubgraphWs(Carve& w, long n) {
    key = w.take_n<u64>(n);
    fr0 = w.take_n<int>(n); fr1 = w.take_n<int>(n);
  }
};

struct InducedSubgraphWs {     // prefix sums of both masks (E >= 1 here), rocPRIM scratch
  int *pv, *pe;
  void* tmp; size_t tmp_bytes;
  InducedSubgraphWs(Carve& w, long n, long E) {
    pv = w.take_n<int>(n);
    pe = w.take_n<int>(E);
    const auto mask = rocprim::make_transform_iterator((const uint8_t*)nullptr, NonZero());
    tmp_bytes = std::max(exclusive_scan_bytes<int>(n, mask), exclusive_scan_bytes<int>(E, mask));
    tmp = w.take(tmp_bytes);
  }
};

__global__ void is_vertices_kernel(const uint8_t* __restrict__ sel, const int* __restrict__ pre, long n, int64_t* __restrict__ rows,
                                   int64_t* __restrict__ new_ver_index, int64_t* __restrict__ counts) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const bool s = sel[v] != 0;
  const int p = pre[v];
  new_ver_index[v] = s ? (int64_t)p : (int64_t)-1;
  if (s) rows[p] = v;
  if (v == n - 1) counts[0] = p + (s ? 1 : 0);
}

__global__ void is_edges_kernel(const uint8_t* __restrict__ sel, const int* __restrict__ pre, long E, const int2* __restrict__ ends,
                                const int64_t* __restrict__ new_ver_index, int64_t* __restrict__ kept, int64_t* __restrict__ src,
                                int64_t* __restrict__ tgt, int64_t* __restrict__ counts) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const bool s = sel[e] != 0;
  const int p = pre[e];
  if (s) {
    const int2 en = ends[e];
    kept[p] = e;
    src[p] = new_ver_index[en.x];
    tgt[p] = new_ver_index[en.y];
  }
  if (e == E - 1) counts[1] = p + (s ? 1 : 0);
}

template <typename IDX>
void launch_tiles(bool stream_stores, dim3 grid, size_t lds, hipStream_t st, const float* xyz, const float* rgb, int cloud_rgb, const void* nei,
                  long K, int k, const int64_t* rows, long m, long N, TileGlobals g, float* clouds, float* clouds_global, float* diameters,
                  int32_t* flag) {
  if (stream_stores)
    hipLaunchKernelGGL((tiles_kernel<IDX, true>), grid, dim3(TL_BLOCK), lds, st, xyz, rgb, cloud_rgb, (const IDX*)nei, K, k, rows, m, N, g, clouds,
                       clouds_global, diameters, flag);
  else
    hipLaunchKernelGGL((tiles_kernel<IDX, false>), grid, dim3(TL_BLOCK), lds, st, xyz, rgb, cloud_rgb, (const IDX*)nei, K, k, rows, m, N, g, clouds,
                       clouds_global, diameters, flag);
}

}  // namespace

extern "C" int spg_neighbourhood_tiles(const float* xyz, const float* rgb, long N, const void* nei, int nei_is_i64, long K, int k,
                                       const int64_t* rows, long m, int cloud_rgb, const float* elevation, const float* xyn, int own_rgb,
                                       int own_xy, int flags, float* clouds, float* clouds_global, float* diameters, int32_t* error_flag,
                                       void* stream) {
  SPG_CHECK_ARG(N >= 1 && N < INT_MAX && m >= 0 && m < INT_MAX, "1 <= N < 2^31 - 1 and 0 <= m < 2^31 - 1");
  SPG_CHECK_ARG(k >= 1 && k <= TL_MAX_K && K >= k, "1 <= k <= 64 and k <= K (nei is [N, K])");
  SPG_CHECK_ARG(xyz && nei && error_flag, "bad argument");
  SPG_CHECK_ARG((!cloud_rgb && !own_rgb) || rgb, "rgb is needed for the colour channels and for the 'rgb' global feature");
  if (m == 0) return 0;
  SPG_CHECK_ARG(clouds && clouds_global && diameters, "bad argument");
  TileGlobals g;
  g.elevation = elevation; g.xyn = xyn; g.own_rgb = own_rgb ? 1 : 0; g.own_xy = own_xy ? 1 : 0;
  g.G = 1 + (elevation ? 1 : 0) + (own_rgb ? 3 : 0) + (xyn ? 2 : 0) + (own_xy ? 2 : 0);
  const int F = cloud_rgb ? 6 : 3;
  const size_t lds = ((size_t)TL_VPB * F * k + (size_t)TL_VPB * 7) * sizeof(float);
  const dim3 grid(spg_cdiv(m, TL_VPB));
  hipStream_t st = (hipStream_t)stream;
  if (nei_is_i64)
    launch_tiles<int64_t>((flags & 1) != 0, grid, lds, st, xyz, rgb, cloud_rgb ? 1 : 0, nei, K, k, rows, m, N, g, clouds, clouds_global, diameters,
                          error_flag);
  else
    launch_tiles<int32_t>((flags & 1) != 0, grid, lds, st, xyz, rgb, cloud_rgb ? 1 : 0, nei, K, k, rows, m, N, g, clouds, clouds_global, diameters,
                          error_flag);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_augment_whole(const float* xyz, const float* rgb, long N, const float* M, const float* ref_point, const float* noise_xyz,
                                 const float* noise_rgb, float* xyz_out, float* rgb_out, void* stream) {
  SPG_CHECK_ARG(N >= 0 && N < INT_MAX && (N == 0 || (xyz && xyz_out)), "bad argument");
  SPG_CHECK_ARG((M == nullptr) == (ref_point == nullptr), "M (host [3, 3]) and ref_point (host [3]) come together");
  SPG_CHECK_ARG(rgb_out == nullptr || rgb != nullptr, "rgb_out needs rgb");
  if (N == 0) return 0;
  AugmentArgs a;
  memset(&a, 0, sizeof(a));
  if (M != nullptr) {
    memcpy(a.M, M, sizeof(a.M));
    memcpy(a.ref, ref_point, sizeof(a.ref));
    a.rotate = 1;
  }
  hipLaunchKernelGGL(augment_kernel, dim3(spg_cdiv(N * 3, TL_BLOCK)), dim3(TL_BLOCK), 0, (hipStream_t)stream, xyz, rgb, N, a, noise_xyz, noise_rgb,
                     xyz_out, rgb_out);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spg_random_subgraph_workspace_bytes(long n) {
  Carve w;
  RandomSubgraphWs l(w, std::max<long>(n, 1));
  return w.used();
}

extern "C" int spg_random_subgraph(const int32_t* rowptr, const uint32_t* inc, const int32_t* ends, long E, long n, int subgraph_size,
                                   const int64_t* seeds, int n_seeds, uint8_t* selected_ver, uint8_t* selected_edg, int64_t* state,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(n >= 1 && n < INT_MAX && E >= 0 && E < INT_MAX / 2, "1 <= n < 2^31 - 1 and 0 <= E < 2^30");
  SPG_CHECK_ARG(subgraph_size >= 0 && subgraph_size <= n, "0 <= subgraph_size <= n");
  SPG_CHECK_ARG(n_seeds >= 0 && (n_seeds == 0 || seeds), "bad seeds");
  SPG_CHECK_ARG(rowptr && selected_ver && state && workspace && (E == 0 || (inc && ends && selected_edg)), "bad argument");
  hipStream_t st = (hipStream_t)stream;
  Carve w(workspace, workspace_bytes);
  RandomSubgraphWs l(w, n);
  u64* key = l.key;
  int *fr0 = l.fr0, *fr1 = l.fr1;
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_random_subgraph_workspace_bytes)");
  SPG_RP(hipMemsetAsync(key, 0xFF, (size_t)n * 8, st));
  hipLaunchKernelGGL(rs_kernel, dim3(1), dim3(RS_BLOCK), 0, st, rowptr, inc, ends, (int)n, subgraph_size, seeds, n_seeds, selected_ver, key, fr0, fr1,
                     state);
  SPG_LAUNCH_CHECK();
  if (E > 0) {
    hipLaunchKernelGGL(rs_edges_kernel, dim3(spg_cdiv(E, TL_BLOCK)), dim3(TL_BLOCK), 0, st, (const int2*)ends, (const uint8_t*)selected_ver, E,
                       selected_edg);
    SPG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" size_t spg_induced_subgraph_workspace_bytes(long n, long E) {
  Carve w;
  InducedSubgraphWs l(w, std::max<long>(n, 1), std::max<long>(E, 1));
  return w.used();
}

extern "C" int spg_induced_subgraph(const int32_t* ends, long E, long n, const uint8_t* selected_ver, const uint8_t* selected_edg,
                                    int64_t* rows, int64_t* new_ver_index, int64_t* kept_edges, int64_t* edg_source, int64_t* edg_target,
                                    int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(n >= 1 && n < INT_MAX && E >= 0 && E < INT_MAX / 2, "1 <= n < 2^31 - 1 and 0 <= E < 2^30");
  SPG_CHECK_ARG(selected_ver && rows && new_ver_index && counts && workspace, "bad argument");
  SPG_CHECK_ARG(E == 0 || (ends && selected_edg && kept_edges && edg_source && edg_target), "bad argument");
  hipStream_t st = (hipStream_t)stream;
  Carve w(workspace, workspace_bytes);
  InducedSubgraphWs l(w, n, std::max<long>(E, 1));
  int *pv = l.pv, *pe = l.pe;
  void* tmp = l.tmp;
  const size_t tmp_bytes = l.tmp_bytes;
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_induced_subgraph_workspace_bytes)");
  SPG_RP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
  size_t b = tmp_bytes;
  SPG_RP(rocprim::exclusive_scan(tmp, b, rocprim::make_transform_iterator(selected_ver, NonZero()), pv, 0, (size_t)n, rocprim::plus<int>(), st));
  hipLaunchKernelGGL(is_vertices_kernel, dim3(spg_cdiv(n, TL_BLOCK)), dim3(TL_BLOCK), 0, st, selected_ver, (const int*)pv, n, rows, new_ver_index,
                     counts);
  SPG_LAUNCH_CHECK();
  if (E == 0) return 0;
  b = tmp_bytes;
  SPG_RP(rocprim::exclusive_scan(tmp, b, rocprim::make_transform_iterator(selected_edg, NonZero()), pe, 0, (size_t)E, rocprim::plus<int>(), st));
  hipLaunchKernelGGL(is_edges_kernel, dim3(spg_cdiv(E, TL_BLOCK)), dim3(TL_BLOCK), 0, st, selected_edg, (const int*)pe, E, (const int2*)ends,
                     (const int64_t*)new_ver_index, kept_edges, edg_source, edg_target, counts);
  SPG_LAUNCH_CHECK();
  return 0;
}
