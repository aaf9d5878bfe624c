// Exact k-nearest-neighbour search over a uniform grid (partition/graphs.py:11-73 compute_graph_nn / compute_graph_nn_2,
// partition/provider.py:681-687 interpolate_labels: sklearn NearestNeighbors(algorithm='kd_tree') in the reference).
//
// Build (reference set, spg_knn_build):
//   minmax_kernel        exact bounding box (ordered-bit atomics);
//   params_kernel        fine cell c0 = extent / 2^21 (or the caller's cell_size), slack of the float32 cell assignment;
//   fine_keys_kernel     fine cell of every point, floor((x - min) / c0) in float32, as a 63-bit Morton key (21 bits per axis);
//   rocPRIM radix sort   points by Morton key; the points are copied into that order as float4 {x, y, z, index bits};
//   split_hist_kernel    for every pair of neighbours in the sorted order the coarsest level at which their keys still differ;
//   level_kernel         the level j (cell W = 2^j c0) whose mean occupancy first reaches KNN_TARGET points per occupied cell --
//                        key >> 3j is the Morton key of the level-j cell, so every level is a contiguous run of the ONE sort;
//   run-length encoding  of key >> 3j: the sorted unique occupied cells and their starts.  Cells are found by binary search over
//                        the unique keys (no hash: nothing to size, deterministic, and the keys a wavefront searches are
//                        neighbours in Morton order, so the searches of one ring share cache lines).
// Query (spg_knn_query):
//   self mode   the queries are the reference points themselves, one wavefront per occupied cell (64 queries at a time);
//   query set   the queries of a bounded chunk get the level-j cell of the reference grid (clamped into it), are sorted by it and
//               grouped by run-length encoding; one wavefront per group.
//   knn_query_kernel<CAP>: all lanes of a wavefront share the query cell.  Chebyshev rings r = 0, 1, 2, ... of cells around it:
//   the lanes look up up to 64 ring cells at once (one binary search each), then walk the non-empty ones; 64 candidates at a time
//   are loaded coalesced (one per lane) and broadcast lane by lane with v_readlane (an SGPR operand: cheaper than an LDS round
//   trip).  Each lane keeps its sorted top-k (float64 key, index) in registers (CAP slots, compile-time indexed: no scratch).
//   A lane stops when its k-th best key is strictly below a conservative lower bound on the squared distance to every cell
//   outside the visited box (DESIGN.md section 4.11a has the argument); the wavefront stops when all lanes have.
// Order: key d2 = (dx*dx + dy*dy) + dz*dz in float64, dx = (double)q.x - (double)p.x, no fused multiply-add; ties by point
// index; in self mode the query point itself is excluded (the reference's dropped first column).  The result does not depend
// on the cell size, the level, or the chunking.
#include <cfloat>
#include <climits>
#include <cstring>

#include "../../include/spg_hip.h"
#include "spg_part.h"

namespace {

constexpr int KNN_BITS = 21;                     // fine cells per axis: 2^21 (3 x 21 = 63-bit Morton keys)
constexpr int KNN_TARGET = 32;                   // aimed-at mean points per occupied cell
constexpr long KNN_QCHUNK = 1L << 22;            // queries per internal chunk (query-set mode)
constexpr int KNN_MAX_K = 47;                    // k + 1 <= 48: the largest register-resident list without scratch
constexpr int KNN_BLOCK = 256;

// written by the device during the build; lives at the start of the workspace
struct KnnParams {
  unsigned mm[6];        // min / max per axis as order-preserving bits
  float lo[3], hi[3];    // exact bounding box
  float c0;              // fine cell size
  int level;             // coarse level j: cell W = 2^j c0
  unsigned fmax[3];      // fine cell of hi (per axis)
  int g[3];              // level-j cells per axis
  unsigned n_cells;      // occupied level-j cells
  unsigned n_qseg;       // query groups of the current chunk
  unsigned counter;      // dynamic work counter of a query launch
  unsigned flag;         // bit 0: a non-finite reference coordinate (the index is unusable)
  unsigned qflag;        // bit 0: a non-finite query coordinate (reset by every spg_knn_query)
  unsigned hist[24];     // split levels of consecutive sorted keys
  double slack;          // bound on |true position - cell box| from the float32 cell assignment and float64 rounding
  long n;                // points
};

__device__ __forceinline__ u64 spread3(unsigned v) {
  u64 x = v & 0x1fffffu;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
__device__ __forceinline__ unsigned compact3(u64 x) {
  x &= 0x1249249249249249ull;
  x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ull;
  x = (x ^ (x >> 4)) & 0x100f00f00f00f00full;
  x = (x ^ (x >> 8)) & 0x1f0000ff0000ffull;
  x = (x ^ (x >> 16)) & 0x1f00000000ffffull;
  x = (x ^ (x >> 32)) & 0x1fffffull;
  return (unsigned)x;
}
__device__ __forceinline__ u64 morton(unsigned x, unsigned y, unsigned z) { return spread3(x) | (spread3(y) << 1) | (spread3(z) << 2); }

// fine cell index along one axis: floor((x - lo) / c0) in float32, clamped into [0, hi_idx]; false for a non-finite x
__device__ __forceinline__ bool fine_index(float x, float lo, float c0, unsigned hi_idx, unsigned& idx) {
  const float t = floorf(__fdiv_rn(__fsub_rn(x, lo), c0));
  if (!(t >= 0.f)) idx = 0;                               // below the box (queries only) or NaN
  else idx = t >= (float)hi_idx ? hi_idx : (unsigned)t;
  return isfinite(x);
}

// ---- the order key: float64 squared distance, (dx*dx + dy*dy) + dz*dz, every operation rounded on its own ----
__device__ __forceinline__ double knn_d2(double qx, double qy, double qz, float px, float py, float pz) {
#pragma clang fp contract(off)
  const double dx = qx - (double)px, dy = qy - (double)py, dz = qz - (double)pz;
  return (dx * dx + dy * dy) + dz * dz;
}

// -------------------------------------------------------------------------------------------------------------------
// build
// -------------------------------------------------------------------------------------------------------------------
__global__ void minmax_kernel(const float* __restrict__ xyz, long n, KnnParams* __restrict__ p) {
  const bool bad = axis_minmax(xyz, n, p->mm);
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&p->flag, 1u);
}

__global__ void params_kernel(KnnParams* __restrict__ p, long n, float cell_size) {
  double ext = 0.0, mag = 0.0;
  for (int d = 0; d < 3; ++d) {
    p->lo[d] = from_ordered(p->mm[d]);
    p->hi[d] = from_ordered(p->mm[3 + d]);
    ext = fmax(ext, (double)p->hi[d] - (double)p->lo[d]);
    mag = fmax(mag, fmax(fabs((double)p->lo[d]), fabs((double)p->hi[d])));
  }
  float c0 = cell_size;
  if (!(c0 > 0.f)) c0 = ext > 0.0 ? (float)(ext * (1.0 + 0x1p-10) * 0x1p-21) : 1.f;
  if (!(c0 >= FLT_MIN)) c0 = FLT_MIN;
  p->c0 = c0;
  p->n = n;
  // floor(fl(fl(x - lo) / c0)) = i implies |(x - lo) - i c0| <= 3u (x - lo) <= 3u ext (u = 2^-24) below / above the cell;
  // 2^-21 ext = 8u ext covers it, 2^-40 (|coordinates| + ext) covers the float64 rounding of the box bounds
  p->slack = 0x1p-21 * ext + 0x1p-40 * (mag + ext);
  const unsigned top = (1u << KNN_BITS) - 1u;
  for (int d = 0; d < 3; ++d) {
    unsigned f;
    fine_index(p->hi[d], p->lo[d], c0, top, f);
    p->fmax[d] = f;
  }
  if (!(ext <= (double)FLT_MAX)) p->flag |= 1u;
}

__global__ void fine_keys_kernel(const float* __restrict__ xyz, long n, const KnnParams* __restrict__ p, u64* __restrict__ keys,
                                 unsigned* __restrict__ idx) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned c[3];
  for (int d = 0; d < 3; ++d) fine_index(xyz[3 * i + d], p->lo[d], p->c0, p->fmax[d], c[d]);
  keys[i] = morton(c[0], c[1], c[2]);
  idx[i] = (unsigned)i;
}

__global__ void gather_points_kernel(const float* __restrict__ xyz, const unsigned* __restrict__ idx, long n, float4* __restrict__ pts) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned j = idx[i];
  pts[i] = make_float4(xyz[3 * (long)j], xyz[3 * (long)j + 1], xyz[3 * (long)j + 2], __uint_as_float(j));
}

__global__ void split_hist_kernel(const u64* __restrict__ keys, long n, KnnParams* __restrict__ p) {
  __shared__ unsigned h[24];
  if (threadIdx.x < 24) h[threadIdx.x] = 0;
  __syncthreads();
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x + 1; i < n; i += (long)gridDim.x * blockDim.x) {
    const u64 x = keys[i] ^ keys[i - 1];
    if (x != 0) atomicAdd(&h[(63 - __clzll((long long)x)) / 3], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 24 && h[threadIdx.x] != 0) atomicAdd(&p->hist[threadIdx.x], h[threadIdx.x]);
}

// level_fixed >= 0: that level (the caller's cell_size); otherwise the first level with >= KNN_TARGET points per occupied cell
__global__ void level_kernel(KnnParams* __restrict__ p, int level_fixed) {
  int j = level_fixed;
  if (j < 0) {
    j = KNN_BITS;
    unsigned long long distinct = 1;                       // occupied cells at level l = 1 + #(splits at level >= l)
    for (int l = KNN_BITS - 1; l >= 0; --l) distinct += p->hist[l];
    for (int l = 0; l < KNN_BITS; ++l) {
      if ((double)p->n >= (double)KNN_TARGET * (double)distinct) { j = l; break; }
      distinct -= p->hist[l];
    }
  }
  p->level = j;
  for (int d = 0; d < 3; ++d) p->g[d] = (int)(p->fmax[d] >> j) + 1;
}

__global__ void coarse_keys_kernel(const u64* __restrict__ fine, long n, const KnnParams* __restrict__ p, u64* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = fine[i] >> (3 * p->level);
}

// level-j cell of every query of a chunk (clamped into the grid), global query index as payload
__global__ void query_keys_kernel(const float* __restrict__ q, long q0, long m, KnnParams* __restrict__ p, u64* __restrict__ keys,
                                  unsigned* __restrict__ idx) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (i < m) {
    unsigned c[3];
    for (int d = 0; d < 3; ++d) bad |= !fine_index(q[3 * (q0 + i) + d], p->lo[d], p->c0, p->fmax[d], c[d]);
    const int j = p->level;
    keys[i] = morton(c[0] >> j, c[1] >> j, c[2] >> j);
    idx[i] = (unsigned)(q0 + i);
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&p->qflag, 1u);
}

// -------------------------------------------------------------------------------------------------------------------
// query
// -------------------------------------------------------------------------------------------------------------------
struct QueryArgs {
  const float4* pts;          // reference points in cell order {x, y, z, original index}
  const u64* ukeys;           // occupied level-j cells, ascending
  const unsigned* ustart;     // their starts in pts (n_cells + 1 entries)
  KnnParams* prm;
  const u64* seg_keys;        // groups of queries sharing a cell: self mode = ukeys
  const unsigned* seg_start;  // self mode = ustart
  const unsigned* nseg;       // self mode = &prm->n_cells
  const unsigned* qidx;       // query-set mode: global query index per sorted position
  const float* qxyz;          // query-set mode: query coordinates [n_query, 3]
  int self, k;
  int32_t* idx_out;
  float* dist_out;
};

__device__ __forceinline__ float rl_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ unsigned rl_u(unsigned v, int l) { return (unsigned)__builtin_amdgcn_readlane((int)v, l); }

__device__ __forceinline__ bool key_less(double da, unsigned ia, double db, unsigned ib) { return da < db || (da == db && ia < ib); }

// cell offset t of Chebyshev ring r (r >= 1: 24 r^2 + 2 cells): z faces, then y faces, then x faces
__device__ __forceinline__ void ring_cell(long t, int r, int& dx, int& dy, int& dz) {
  const long s = 2 * r + 1, s2 = s * s;
  if (t < 2 * s2) {
    dz = t < s2 ? -r : r;
    const long u = t < s2 ? t : t - s2;
    dy = (int)(u / s) - r; dx = (int)(u % s) - r;
    return;
  }
  t -= 2 * s2;
  const long f = s * (s - 2);
  if (t < 2 * f) {
    dy = t < f ? -r : r;
    const long u = t < f ? t : t - f;
    dz = (int)(u / s) - r + 1; dx = (int)(u % s) - r;
    return;
  }
  t -= 2 * f;
  const long e = (s - 2) * (s - 2);
  dx = t < e ? -r : r;
  const long u = t < e ? t : t - e;
  dy = (int)(u / (s - 2)) - r + 1; dz = (int)(u % (s - 2)) - r + 1;
}

template <int CAP>
__global__ __launch_bounds__(KNN_BLOCK) void knn_query_kernel(QueryArgs a) {
  const int lane = threadIdx.x & 63;
  const KnnParams* p = a.prm;
  if ((p->flag | p->qflag) & 1u) return;                     // non-finite input: the caller raises
  const unsigned nseg = *a.nseg, n_cells = p->n_cells;
  const int level = p->level, k = a.k;
  const double W = ldexp((double)p->c0, level), slack = p->slack;
  double lo[3], hi[3];
  int g[3];
  for (int d = 0; d < 3; ++d) { lo[d] = p->lo[d]; hi[d] = p->hi[d]; g[d] = p->g[d]; }
  const double round_down = 1.0 - 0x1p-40;

  for (;;) {
    unsigned seg = 0;
    if (lane == 0) seg = atomicAdd(&a.prm->counter, 1u);
    seg = rl_u(seg, 0);
    if (seg >= nseg) break;
    const unsigned s0 = a.seg_start[seg], s1 = a.seg_start[seg + 1];
    const u64 key = a.seg_keys[seg];
    const int c[3] = {(int)compact3(key), (int)compact3(key >> 1), (int)compact3(key >> 2)};

    for (unsigned q0 = s0; q0 < s1; q0 += 64) {
      const unsigned qi = q0 + lane;
      const bool active = qi < s1;
      double q[3] = {0.0, 0.0, 0.0};
      unsigned qid = 0;
      if (active) {
        if (a.self) {
          const float4 v = a.pts[qi];
          q[0] = v.x; q[1] = v.y; q[2] = v.z; qid = __float_as_uint(v.w);
        } else {
          qid = a.qidx[qi];
          q[0] = a.qxyz[3 * (long)qid]; q[1] = a.qxyz[3 * (long)qid + 1]; q[2] = a.qxyz[3 * (long)qid + 2];
        }
      }
      const unsigned skip = a.self ? qid : 0xffffffffu;
      // slots [0, CAP - k) hold a sentinel below every key; the k real entries are [CAP - k, CAP), ascending
      double bd[CAP];
      unsigned bi[CAP];
#pragma unroll
      for (int i = 0; i < CAP; ++i) { bd[i] = i < CAP - k ? -1.0 : (double)INFINITY; bi[i] = 0xffffffffu; }
      // squared distance of the query to the bounding box along each axis (zero inside); bound slack per query
      double o2[3], dq = slack;
      for (int d = 0; d < 3; ++d) {
        const double o = fmax(0.0, fmax(lo[d] - q[d], q[d] - hi[d]));
        o2[d] = o * o;
        dq = fmax(dq, slack + 0x1p-40 * fabs(q[d]));
      }
      bool done = !active || !(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]));

      for (int r = 0; __any(!done); ++r) {
        const long nshell = r == 0 ? 1 : 24L * r * r + 2;
        bool ring_occupied = false;
        for (long t0 = 0; t0 < nshell; t0 += 64) {
          const long t = t0 + lane;
          int cc[3] = {c[0], c[1], c[2]};
          bool ok = t < nshell;
          if (ok && r > 0) {
            int dx, dy, dz;
            ring_cell(t, r, dx, dy, dz);
            cc[0] += dx; cc[1] += dy; cc[2] += dz;
          }
          ok = ok && cc[0] >= 0 && cc[0] < g[0] && cc[1] >= 0 && cc[1] < g[1] && cc[2] >= 0 && cc[2] < g[2];
          unsigned cs = 0, cn = 0;
          if (ok) {
            const u64 m = morton((unsigned)cc[0], (unsigned)cc[1], (unsigned)cc[2]);
            unsigned lo_i = 0, hi_i = n_cells;
            while (lo_i < hi_i) {
              const unsigned mid = (lo_i + hi_i) >> 1;
              if (a.ukeys[mid] < m) lo_i = mid + 1; else hi_i = mid;
            }
            if (lo_i < n_cells && a.ukeys[lo_i] == m) { cs = a.ustart[lo_i]; cn = a.ustart[lo_i + 1] - cs; }
          }
          u64 mask = __ballot(cn != 0);
          ring_occupied = ring_occupied || mask != 0;
          while (mask != 0) {
            const int b = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const unsigned s = rl_u(cs, b), e = s + rl_u(cn, b);
            // lower bound of this lane's squared distance to any point of the cell: skip the cell if it cannot enter
            double lb = 0.0;
            for (int d = 0; d < 3; ++d) {
              const int cd = __builtin_amdgcn_readlane(cc[d], b);
              const double blo = lo[d] + (double)cd * W - dq;
              double bhi = lo[d] + (double)(cd + 1) * W + dq;
              if (cd == g[d] - 1) bhi = fmax(bhi, hi[d]);
              const double gap = fmax(0.0, fmax(blo - q[d], q[d] - bhi));
              lb += gap * gap;
            }
            const bool want = !done && lb * round_down <= bd[CAP - 1];
            if (!__any(want)) continue;
            for (unsigned p0 = s; p0 < e; p0 += 64) {
              float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
              if (p0 + lane < e) v = a.pts[p0 + lane];
              const int cnt = (int)min(64u, e - p0);
#pragma unroll 1
              for (int j = 0; j < cnt; ++j) {
                const float px = rl_f(v.x, j), py = rl_f(v.y, j), pz = rl_f(v.z, j);
                const unsigned pid = rl_u(__float_as_uint(v.w), j);
                const double dc = knn_d2(q[0], q[1], q[2], px, py, pz);
                const unsigned ic = pid;
                // sorted insertion from the top, in place: slot i takes slot i-1 when the candidate precedes both, the
                // candidate when it precedes slot i only; the last entry drops out.  Predicated, under a wave-uniform
                // branch: no divergent control flow around the register-resident list.
                bool lt_hi = want && pid != skip && key_less(dc, ic, bd[CAP - 1], bi[CAP - 1]);
                if (__any(lt_hi)) {
#pragma unroll
                  for (int i = CAP - 1; i > 0; --i) {
                    const bool lt_lo = key_less(dc, ic, bd[i - 1], bi[i - 1]);
                    bd[i] = lt_hi ? (lt_lo ? bd[i - 1] : dc) : bd[i];
                    bi[i] = lt_hi ? (lt_lo ? bi[i - 1] : ic) : bi[i];
                    lt_hi = lt_hi && lt_lo;
                  }
                  bd[0] = lt_hi ? dc : bd[0];
                  bi[0] = lt_hi ? ic : bi[0];
                }
              }
            }
          }
        }
        // an empty ring that costs more lookups than a scan of the occupied cells (an isolated point, a query beside the cloud):
        // jump to the ring before the nearest occupied cell -- the rings in between hold no point, so nothing is skipped
        if (!ring_occupied && r >= 2 && nshell * 16 >= (long)n_cells) {
          int rn = INT_MAX;
          for (unsigned i = lane; i < n_cells; i += 64) {
            const u64 key = a.ukeys[i];
            const int cheb = max(max(abs((int)compact3(key) - c[0]), abs((int)compact3(key >> 1) - c[1])), abs((int)compact3(key >> 2) - c[2]));
            if (cheb > r) rn = min(rn, cheb);
          }
          for (int o = 32; o >= 1; o >>= 1) rn = min(rn, __shfl_xor(rn, o, 64));
          // no occupied cell beyond ring r: every cell has been seen; a ring that covers the grid leaves no slab below
          r = rn == INT_MAX ? max(max(max(c[0], g[0] - 1 - c[0]), max(c[1], g[1] - 1 - c[1])), max(c[2], g[2] - 1 - c[2])) : rn - 1;
        }
        // every cell with Chebyshev distance <= r is visited (or was skipped by its own bound): the unvisited points lie in a
        // slab below c - r or above c + r along some axis that the grid still has
        double lb2 = (double)INFINITY;
        for (int d = 0; d < 3; ++d) {
          const double other = o2[0] + o2[1] + o2[2] - o2[d];
          if (c[d] - r > 0) {
            const double gap = fmax(0.0, q[d] - (lo[d] + (double)(c[d] - r) * W + dq));
            lb2 = fmin(lb2, gap * gap + other);
          }
          if (c[d] + r < g[d] - 1) {
            const double gap = fmax(0.0, (lo[d] + (double)(c[d] + r + 1) * W - dq) - q[d]);
            lb2 = fmin(lb2, gap * gap + other);
          }
        }
        if (!done) done = lb2 == (double)INFINITY || bd[CAP - 1] < lb2 * round_down;
      }

      if (active) {
        const long row = (long)qid * k - (CAP - k);
#pragma unroll
        for (int i = 0; i < CAP; ++i) {
          if (i >= CAP - k) {
            a.idx_out[row + i] = (int32_t)bi[i];
            if (a.dist_out != nullptr) a.dist_out[row + i] = (float)__dsqrt_rn(bd[i]);
          }
        }
      }
    }
  }
}

// sort + run-length buffers for m keys (the build and every query chunk use the same shape; only a query chunk keeps its cells)
struct SegWs {
  u64 *k0, *k1, *ukeys;
  unsigned *i0, *i1, *counts, *start;
  void* tmp; size_t tmp_bytes;
  SegWs(Carve& w, long m, bool with_cells) {
    k0 = w.take_n<u64>(m); k1 = w.take_n<u64>(m);
    ukeys = with_cells ? w.take_n<u64>(m) : nullptr;
    i0 = w.take_n<unsigned>(m); i1 = w.take_n<unsigned>(m);
    counts = w.take_n<unsigned>(m + 1);
    start = with_cells ? w.take_n<unsigned>(m + 1) : nullptr;
    tmp_bytes = std::max({radix_sort_pairs_bytes<u64, unsigned>(m, 0, 63), run_length_encode_bytes<u64, unsigned>(m),
                          exclusive_scan_bytes<unsigned>(m + 1)});
    tmp = w.take(tmp_bytes);
  }
};
size_t seg_bytes(long m, bool with_cells) { Carve w; SegWs s(w, m, with_cells); return w.used(); }

// persistent part: parameters, points in cell order, occupied cells and their starts; the build and the query chunks carve the rest
struct KnnWs {
  KnnParams* prm;
  float4* pts;
  u64* ukeys;
  unsigned* ustart;
  KnnWs(Carve& w, long n) {
    prm = w.take_n<KnnParams>(1);
    pts = w.take_n<float4>(n);
    ukeys = w.take_n<u64>(n);
    ustart = w.take_n<unsigned>(n + 1);
  }
};
size_t persistent_bytes(long n) { Carve w; KnnWs k(w, n); return w.used(); }

__global__ void error_out_kernel(const KnnParams* __restrict__ p, int32_t* __restrict__ out) { *out = (int32_t)(p->flag | p->qflag); }

// queries per internal chunk: min(n_query, KNN_QCHUNK), halved until its sort / run-length scratch fits what the workspace
// leaves after the persistent part; 0 when not even 64 queries fit
long query_chunk(size_t scratch_bytes, long n_query) {
  long m = std::min(n_query, KNN_QCHUNK);
  while (m > 64 && seg_bytes(m, true) > scratch_bytes) m = (m + 1) / 2;
  return seg_bytes(m, true) <= scratch_bytes ? m : 0;
}

int launch_query(const QueryArgs& a, long max_groups, hipStream_t st) {
  const int grid = (int)std::min<long>(std::max<long>(spg_cdiv(max_groups, KNN_BLOCK / 64), 1), 1024);
  SPG_RP(hipMemsetAsync(&a.prm->counter, 0, sizeof(unsigned), st));
#define KNN_LAUNCH(C) hipLaunchKernelGGL(knn_query_kernel<C>, dim3(grid), dim3(KNN_BLOCK), 0, st, a)
  const int k = a.k;
  if (k <= 1) KNN_LAUNCH(1);
  else if (k <= 2) KNN_LAUNCH(2);
  else if (k <= 4) KNN_LAUNCH(4);
  else if (k <= 8) KNN_LAUNCH(8);
  else if (k <= 16) KNN_LAUNCH(16);
  else if (k <= 32) KNN_LAUNCH(32);
  else KNN_LAUNCH(48);
#undef KNN_LAUNCH
  SPG_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" size_t spg_knn_workspace_bytes(long n_ref, long n_query, int k) {
  (void)k;
  if (n_ref < 1) n_ref = 1;
  if (n_query < 0) n_query = 0;
  const long m = std::min(n_query, KNN_QCHUNK);      // the larger of the build layout and the layout of a full query chunk
  return persistent_bytes(n_ref) + std::max(seg_bytes(n_ref, false), m > 0 ? seg_bytes(m, true) : 0);
}

extern "C" int spg_knn_build(const float* ref_xyz, long n_ref, float cell_size, int32_t* error_flag, void* workspace,
                             size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(ref_xyz && workspace && n_ref > 0, "bad argument");
  SPG_CHECK_ARG(n_ref < (1L << 32) - 1, "more than 2^32 - 2 reference points (indices are uint32)");
  SPG_CHECK_ARG(!(cell_size < 0.f) && !(cell_size > FLT_MAX), "cell_size must be >= 0 and finite (0 = automatic)");
  hipStream_t st = (hipStream_t)stream;
  Carve w(workspace, workspace_bytes);
  KnnWs k(w, n_ref);
  SegWs s(w, n_ref, false);
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_knn_workspace_bytes)");
  const long n = n_ref;
  const dim3 block(256), grid(spg_cdiv(n, 256));
  SPG_RP(hipMemsetAsync(k.prm, 0, sizeof(KnnParams), st));
  SPG_RP(hipMemsetAsync(k.prm->mm, 0xff, 3 * sizeof(unsigned), st));      // running minima (ordered bits): all ones
  hipLaunchKernelGGL(minmax_kernel, dim3(n < 262144 ? spg_cdiv(n, 256) : 1024), block, 0, st, ref_xyz, n, k.prm);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(params_kernel, dim3(1), dim3(1), 0, st, k.prm, n, cell_size);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(fine_keys_kernel, grid, block, 0, st, ref_xyz, n, (const KnnParams*)k.prm, s.k0, s.i0);
  SPG_LAUNCH_CHECK();
  size_t b = s.tmp_bytes;
  SPG_RP(rocprim::radix_sort_pairs(s.tmp, b, (const u64*)s.k0, s.k1, (const unsigned*)s.i0, s.i1, (size_t)n, 0, 3 * KNN_BITS, st));
  hipLaunchKernelGGL(gather_points_kernel, grid, block, 0, st, ref_xyz, (const unsigned*)s.i1, n, k.pts);
  SPG_LAUNCH_CHECK();
  if (cell_size > 0.f) {
    hipLaunchKernelGGL(level_kernel, dim3(1), dim3(1), 0, st, k.prm, 0);
  } else {
    hipLaunchKernelGGL(split_hist_kernel, dim3(std::min(spg_cdiv(n, 256), 1024)), block, 0, st, (const u64*)s.k1, n, k.prm);
    SPG_LAUNCH_CHECK();
    hipLaunchKernelGGL(level_kernel, dim3(1), dim3(1), 0, st, k.prm, -1);
  }
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(coarse_keys_kernel, grid, block, 0, st, (const u64*)s.k1, n, (const KnnParams*)k.prm, s.k0);
  SPG_LAUNCH_CHECK();
  SPG_RP(hipMemsetAsync(s.counts, 0, (size_t)(n + 1) * 4, st));
  b = s.tmp_bytes;
  SPG_RP(rocprim::run_length_encode(s.tmp, b, (const u64*)s.k0, (unsigned)n, k.ukeys, s.counts, &k.prm->n_cells, st));
  b = s.tmp_bytes;
  SPG_RP(rocprim::exclusive_scan(s.tmp, b, (const unsigned*)s.counts, k.ustart, 0u, (size_t)(n + 1), rocprim::plus<unsigned>(), st));
  if (error_flag != nullptr) SPG_RP(hipMemcpyAsync(error_flag, &k.prm->flag, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return 0;
}

extern "C" int spg_knn_query(const float* query_xyz, long n_query, long n_ref, int k, int self_query, int32_t* idx_out, float* dist_out,
                             int32_t* error_flag, void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(workspace && idx_out && n_ref > 0 && n_ref < (1L << 32) - 1, "bad argument");
  SPG_CHECK_ARG(k >= 1 && k <= KNN_MAX_K, "k must be in [1, 47] (k + 1 <= 48)");
  SPG_CHECK_ARG(self_query ? (n_query == n_ref && k < n_ref) : (n_query >= 0 && n_query < (1L << 32) - 1 && k <= n_ref && (n_query == 0 || query_xyz)),
                "self query: n_query == n_ref > k; query set: k <= n_ref");
  hipStream_t st = (hipStream_t)stream;
  Carve c(workspace, workspace_bytes);
  KnnWs w(c, n_ref);
  SPG_CHECK_ARG(c.ok, "workspace too small (spg_knn_workspace_bytes)");
  SPG_RP(hipMemsetAsync(&w.prm->qflag, 0, sizeof(unsigned), st));
  QueryArgs a{};
  a.pts = w.pts; a.ukeys = w.ukeys; a.ustart = w.ustart; a.prm = w.prm;
  a.k = k; a.idx_out = idx_out; a.dist_out = dist_out; a.self = self_query ? 1 : 0;
  if (self_query) {
    a.seg_keys = w.ukeys; a.seg_start = w.ustart; a.nseg = &w.prm->n_cells;
    SPG_TRY(launch_query(a, n_ref, st));
  } else if (n_query > 0) {
    const long m = query_chunk(c.left(), n_query);
    SPG_CHECK_ARG(m > 0, "workspace too small for a query chunk (spg_knn_workspace_bytes)");
    SegWs s(c, m, true);
    SPG_CHECK_ARG(c.ok, "workspace too small for a query chunk (spg_knn_workspace_bytes)");
    a.qxyz = query_xyz; a.qidx = s.i1; a.seg_keys = s.ukeys; a.seg_start = s.start; a.nseg = &w.prm->n_qseg;
    for (long q0 = 0; q0 < n_query; q0 += m) {
      const long mc = std::min(m, n_query - q0);
      hipLaunchKernelGGL(query_keys_kernel, dim3(spg_cdiv(mc, 256)), dim3(256), 0, st, query_xyz, q0, mc, w.prm, s.k0, s.i0);
      SPG_LAUNCH_CHECK();
      size_t b = s.tmp_bytes;
      SPG_RP(rocprim::radix_sort_pairs(s.tmp, b, (const u64*)s.k0, s.k1, (const unsigned*)s.i0, s.i1, (size_t)mc, 0, 3 * KNN_BITS, st));
      SPG_RP(hipMemsetAsync(s.counts, 0, (size_t)(mc + 1) * 4, st));
      b = s.tmp_bytes;
      SPG_RP(rocprim::run_length_encode(s.tmp, b, (const u64*)s.k1, (unsigned)mc, s.ukeys, s.counts, &w.prm->n_qseg, st));
      b = s.tmp_bytes;
      SPG_RP(rocprim::exclusive_scan(s.tmp, b, (const unsigned*)s.counts, s.start, 0u, (size_t)(mc + 1), rocprim::plus<unsigned>(), st));
      SPG_TRY(launch_query(a, mc, st));
    }
  }
  if (error_flag != nullptr) {
    hipLaunchKernelGGL(error_out_kernel, dim3(1), dim3(1), 0, st, (const KnnParams*)w.prm, error_flag);
    SPG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" long spg_knn_query_chunk(long n_ref, long n_query, size_t workspace_bytes) {
  if (n_ref < 1 || n_query < 1) return 0;
  const size_t persistent = persistent_bytes(n_ref);
  return workspace_bytes > persistent ? query_chunk(workspace_bytes - persistent, n_query) : 0;
}
