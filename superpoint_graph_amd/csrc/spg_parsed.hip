// "Reorganize point clouds into superpoints" on the device: the per-scene body of the reference's preprocess_pointclouds
// (learning/s3dis_dataset.py:93-162, sema3d_dataset.py:85-135, vkitti_dataset.py:83-130, custom_dataset.py:67-107), restated
// (tests/parsed_restatement.py is the same text in numpy).  Three entry points:
//
// spg_parsed_stats   the scene statistics by the fixed-order reduction of spg_part.h (the same input gives the same bits).  Pass 0:
//                    min / max per axis in float32, the sums of x, y, z in float64, the finite check.  Passes 1, 2 (S3DIS only): the
//                    sum of d = sqrt((x - cx)^2 + (y - cy)^2), then of (d - mean d)^2, in float64 (numpy's two-pass std, ddof = 0).
// spg_parsed_rows    one pass: output row r -> its superpoint by bisection of the output offsets -> its source vertex through the
//                    component list (and the trim table) -> the columns of the recipe, into LDS; the workgroup's PR_ROWS rows leave
//                    as ONE contiguous span of 16-byte non-temporal stores (rows of 11 / 14 / 15 floats are not 16-byte aligned,
//                    a span of 256 rows is).
// spg_class_count    bincount(argmax(labels[:, 1:], 1)): first maximum, integer atomics (LDS, then one per class and workgroup).
//
// The float32 steps are the reference's, operation by operation, with contraction off; the divisions go through float64 (53 >= 2 * 24
// + 2 bits: rounding the float64 quotient once more to float32 cannot differ from rounding the exact one).
// Error word: bit 0 a coordinate is NaN / infinite, bit 1 a component index outside [0, n), bit 2 a trim position outside [0, size).
#include <climits>
#include <cmath>
#include <cstring>

#include "../../include/spg_hip.h"
#include "spg_part.h"

namespace {

constexpr int PR_BLOCK = PART_BLOCK;
constexpr int PR_ROWS = PR_BLOCK;        // output rows per workgroup of the row pass: one per lane
constexpr int PR_MAX_COLS = 15;
constexpr int PR_MAX_CLASSES = 4096;     // the LDS histogram of the class count

// stats_f32 [6]: min x, y, z, max x, y, z.  stats_f64 [5]: mean x, y, z, mean d, std d.
__device__ __forceinline__ float div_rn_f32(float a, float b) { return (float)((double)a / (double)b); }

__device__ __forceinline__ double centre_distance(const float* __restrict__ xyz, long i, double cx, double cy) {
#pragma clang fp contract(off)
  const double dx = (double)xyz[3 * i] - cx, dy = (double)xyz[3 * i + 1] - cy;
  const double xx = dx * dx, yy = dy * dy;
  return sqrt(xx + yy);
}

// The passes (spg_part.h) of the scene statistics.  Pass 0: v[0..2] min, v[3..5] max, v[6..8] sums of x, y, z, and the finite check.
struct StatsPass0 {
  typedef double T;
  static constexpr int K = 9;
  static constexpr int op(int c) { return c < 3 ? PART_MIN : c < 6 ? PART_MAX : PART_SUM; }
  float* stats_f32;
  double* stats_f64;
  float* centroid;
  __device__ void point(const float* __restrict__ xyz, long i, double (&v)[9], int& bad) const {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = xyz[3 * i + c];
      bad |= !finite_f32(x);
      v[c] = fmin(v[c], (double)x);
      v[3 + c] = fmax(v[3 + c], (double)x);
      v[6 + c] += (double)x;
    }
  }
  __device__ void write(const double (&v)[9], long n) const {
#pragma unroll
    for (int c = 0; c < 6; ++c) stats_f32[c] = (float)v[c];        // (exact: the minimum of float32 values)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double m = v[6 + c] / (double)n;
      stats_f64[c] = m;
      centroid[c] = (float)m;
    }
    stats_f64[3] = NAN; stats_f64[4] = NAN;
  }
};

// SQUARED false: the sum of d -> stats_f64[3] = mean d.  SQUARED true: the sum of (d - mean d)^2 -> stats_f64[4] = std d.
template <bool SQUARED>
struct DistancePass {
  typedef double T;
  static constexpr int K = 1;
  static constexpr int op(int) { return PART_SUM; }
  double* stats_f64;
  __device__ void point(const float* __restrict__ xyz, long i, double (&v)[1], int&) const {
#pragma clang fp contract(off)
    const double d = centre_distance(xyz, i, stats_f64[0], stats_f64[1]);
    const double t = d - stats_f64[3];
    v[0] += SQUARED ? t * t : d;
  }
  __device__ void write(const double (&v)[1], long n) const {
    const double m = v[0] / (double)n;
    stats_f64[SQUARED ? 4 : 3] = SQUARED ? sqrt(m) : m;
  }
};

// ---- rows --------------------------------------------------------------------------------------------------------------
struct RowArgs {
  int recipe, ncols;             // SPG_PARSED_*
  const float* xyz;
  long n;
  const void* rgb;
  int rgb_is_f32;
  const float* geof;             // [n, 4] or null (vkitti)
  const float* elevation;        // [n] or null: s3dis takes z / 4 - 0.5 then
  int lpsv_raw;                  // s3dis: geof unchanged (supervized_partition)
  const float* stats_f32;
  const double* stats_f64;
  const int64_t *out_off, *src_off;   // [C + 1]
  long C;
  const void* comp_idx;
  int idx_is_i64;
  const int32_t* trim;           // [n_trim] positions inside a component
  const int64_t* trim_off;       // [C]: first entry of the component's selection, -1 = not trimmed; null = nothing is trimmed
  long n_rows;
  float* points;
};

__device__ __forceinline__ float rgb_value(const RowArgs& a, long v, int c) {
#pragma clang fp contract(off)
  const double raw = a.rgb_is_f32 ? (double)((const float*)a.rgb)[3 * v + c] : (double)((const uint8_t*)a.rgb)[3 * v + c];
  const double q = raw / 255.0;
  return (float)(q - 0.5);
}

__global__ __launch_bounds__(PR_BLOCK) void rows_kernel(RowArgs a, int32_t* __restrict__ err) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float rows[PR_ROWS * PR_MAX_COLS];
  const long r0 = (long)blockIdx.x * PR_ROWS;
  const long r = r0 + threadIdx.x;
  const int nr = (int)min((long)PR_ROWS, a.n_rows - r0);
  if (r < a.n_rows) {
    long lo = 0, hi = a.C;                             // the last c with out_off[c] <= r: empty components are stepped over
    while (hi - lo > 1) {
      const long mid = (lo + hi) >> 1;
      if (a.out_off[mid] <= r) lo = mid; else hi = mid;
    }
    const long c = lo, j = r - a.out_off[c];
    const long s0 = a.src_off[c], size = a.src_off[c + 1] - s0;
    long pos = j;
    int bad = 0;
    const long t0 = a.trim_off != nullptr ? a.trim_off[c] : -1;
    if (t0 >= 0) {
      pos = a.trim[t0 + j];
      if (pos < 0 || pos >= size) { bad |= 4; pos = 0; }
    }
    long v = a.idx_is_i64 ? ((const int64_t*)a.comp_idx)[s0 + pos] : (long)((const int32_t*)a.comp_idx)[s0 + pos];
    if (v < 0 || v >= a.n) { bad |= 2; v = 0; }
    if (bad) atomicOr(err, bad);

    float* o = rows + threadIdx.x * a.ncols;
    const float x = a.xyz[3 * v], y = a.xyz[3 * v + 1], z = a.xyz[3 * v + 2];
    o[0] = x; o[1] = y; o[2] = z;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[3 + k] = rgb_value(a, v, k);
    if (a.recipe == SPG_PARSED_SEMA3D) {
      o[6] = div_rn_f32(z, 100.f);
#pragma unroll
      for (int k = 0; k < 4; ++k) o[7 + k] = a.geof[4 * v + k] - 0.5f;
    } else if (a.recipe == SPG_PARSED_S3DIS) {
      if (a.elevation != nullptr) {
        o[6] = a.elevation[v];
      } else {
        const float q = z / 4.f;
        o[6] = q - 0.5f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float g = a.geof[4 * v + k];
        o[7 + k] = a.lpsv_raw ? g : g - 0.5f;
      }
      const float p[3] = {x, y, z};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float mi = a.stats_f32[k], ma = a.stats_f32[3 + k];
        const float num = p[k] - mi, ext = ma - mi;
        const float den = ext + 1e-8f;
        o[11 + k] = div_rn_f32(num, den);
      }
      const double d = centre_distance(a.xyz, v, a.stats_f64[0], a.stats_f64[1]);
      const double t = d - a.stats_f64[3];
      o[14] = (float)(t / a.stats_f64[4]);
    } else {                                           // vkitti
      const float mi = a.stats_f32[2], ma = a.stats_f32[5];
      const float num = z - mi, ext = ma - mi;
      const float q = div_rn_f32(num, ext);
      o[6] = q - 0.5f;
      o[7] = 0.f; o[8] = 0.f; o[9] = 0.f; o[10] = 0.f;
      const double tx = (double)x - 30.0, ty = (double)y - 0.0, tz = (double)z - 0.0;
      o[11] = (float)(tx / 30.0); o[12] = (float)(ty / 5.0); o[13] = (float)(tz / 3.0);
    }
  }
  __syncthreads();
  // the span of this workgroup: floats [r0 * ncols, (r0 + nr) * ncols); r0 is a multiple of 256, so the span starts 16-byte aligned
  const int total = nr * a.ncols, quads = total >> 2;
  float* out = a.points + r0 * a.ncols;
  for (int q = threadIdx.x; q < quads; q += PR_BLOCK)
    __builtin_nontemporal_store(reinterpret_cast<const f32x4*>(rows)[q], reinterpret_cast<f32x4*>(out) + q);
  for (int i = 4 * quads + threadIdx.x; i < total; i += PR_BLOCK) __builtin_nontemporal_store(rows[i], out + i);
}

// ---- class count -------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(PR_BLOCK) void class_count_kernel(const T* __restrict__ labels, long n, int n_classes, u64* __restrict__ count) {
  __shared__ unsigned hist[PR_MAX_CLASSES];
  for (int c = threadIdx.x; c < n_classes; c += PR_BLOCK) hist[c] = 0u;
  __syncthreads();
  const int ld = n_classes + 1;
  for (long i = (long)blockIdx.x * PR_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * PR_BLOCK) {
    const T* row = labels + i * ld + 1;
    int best = 0;
    T top = row[0];
    for (int c = 1; c < n_classes; ++c) {
      const T x = row[c];
      if (x > top) { top = x; best = c; }              // strictly greater: the first maximum
    }
    atomicAdd(&hist[best], 1u);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < n_classes; c += PR_BLOCK)
    if (hist[c] != 0u) atomicAdd(&count[c], (u64)hist[c]);
}

// ---- workspace ---------------------------------------------------------------------------------------------------------
struct StatsWs {
  double* partials;          // [blocks, 9]
  int blocks;
  StatsWs(Carve& w, long n) {
    blocks = part_reduce_blocks(n);
    partials = w.take_n<double>((size_t)blocks * 9);
  }
};

}  // namespace

extern "C" size_t spg_parsed_workspace_bytes(long n) {
  Carve w;
  StatsWs l(w, n);
  return w.used();
}

extern "C" int spg_parsed_stats(const float* xyz, long n, int with_distance, float* stats_f32, double* stats_f64, float* centroid,
                                int32_t* error_flag, void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(xyz && stats_f32 && stats_f64 && centroid && error_flag && workspace, "bad argument");
  SPG_CHECK_ARG(n >= 1 && n < INT_MAX, "1 <= n < 2^31 - 1");
  Carve w(workspace, workspace_bytes);
  StatsWs l(w, n);
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_parsed_workspace_bytes(n))");
  hipStream_t st = (hipStream_t)stream;
  SPG_RP(hipMemsetAsync(error_flag, 0, sizeof(int32_t), st));
  if (int rc = part_reduce(StatsPass0{stats_f32, stats_f64, centroid}, xyz, n, l.partials, l.blocks, error_flag, st)) return rc;
  if (with_distance) {
    if (int rc = part_reduce(DistancePass<false>{stats_f64}, xyz, n, l.partials, l.blocks, nullptr, st)) return rc;
    if (int rc = part_reduce(DistancePass<true>{stats_f64}, xyz, n, l.partials, l.blocks, nullptr, st)) return rc;
  }
  return 0;
}

extern "C" int spg_parsed_rows(int recipe, const float* xyz, long n, const void* rgb, int rgb_is_f32, const float* geof, const float* elevation,
                               int lpsv_raw, const float* stats_f32, const double* stats_f64, const int64_t* out_off, const int64_t* src_off,
                               long n_comp, const void* comp_idx, int idx_is_i64, const int32_t* trim, const int64_t* trim_off, long n_rows,
                               float* points, int32_t* error_flag, void* stream) {
  SPG_CHECK_ARG(recipe == SPG_PARSED_S3DIS || recipe == SPG_PARSED_SEMA3D || recipe == SPG_PARSED_VKITTI, "unknown recipe");
  SPG_CHECK_ARG(xyz && rgb && out_off && src_off && error_flag, "bad argument");
  SPG_CHECK_ARG(n >= 1 && n < INT_MAX && n_comp >= 1 && n_rows >= 0 && n_rows < INT_MAX, "1 <= n < 2^31 - 1, n_comp >= 1, 0 <= n_rows < 2^31 - 1");
  SPG_CHECK_ARG(recipe == SPG_PARSED_VKITTI || geof, "the recipe needs geof");
  SPG_CHECK_ARG(recipe == SPG_PARSED_SEMA3D || (stats_f32 && stats_f64), "the recipe needs the scene statistics");
  SPG_CHECK_ARG((trim == nullptr) == (trim_off == nullptr), "trim and trim_off go together");
  if (n_rows == 0) return 0;
  SPG_CHECK_ARG(comp_idx && points, "bad argument");
  RowArgs a;
  a.recipe = recipe;
  a.ncols = recipe == SPG_PARSED_S3DIS ? 15 : recipe == SPG_PARSED_SEMA3D ? 11 : 14;
  a.xyz = xyz; a.n = n; a.rgb = rgb; a.rgb_is_f32 = rgb_is_f32; a.geof = geof;
  a.elevation = recipe == SPG_PARSED_S3DIS ? elevation : nullptr;
  a.lpsv_raw = lpsv_raw;
  a.stats_f32 = stats_f32; a.stats_f64 = stats_f64;
  a.out_off = out_off; a.src_off = src_off; a.C = n_comp;
  a.comp_idx = comp_idx; a.idx_is_i64 = idx_is_i64; a.trim = trim; a.trim_off = trim_off;
  a.n_rows = n_rows; a.points = points;
  hipLaunchKernelGGL(rows_kernel, dim3(spg_cdiv(n_rows, PR_ROWS)), dim3(PR_BLOCK), 0, (hipStream_t)stream, a, error_flag);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_class_count(const void* labels, int labels_signed, long n, int n_classes, int64_t* count, void* stream) {
  SPG_CHECK_ARG(count && (labels || n == 0), "bad argument");
  SPG_CHECK_ARG(n >= 0 && n < INT_MAX && n_classes >= 1 && n_classes <= PR_MAX_CLASSES, "0 <= n < 2^31 - 1, 1 <= n_classes <= 4096");
  hipStream_t st = (hipStream_t)stream;
  SPG_RP(hipMemsetAsync(count, 0, sizeof(int64_t) * (size_t)n_classes, st));
  if (n == 0) return 0;
  const dim3 grid(part_reduce_blocks(n)), blk(PR_BLOCK);
  if (labels_signed) hipLaunchKernelGGL(class_count_kernel<int32_t>, grid, blk, 0, st, (const int32_t*)labels, n, n_classes, (u64*)count);
  else hipLaunchKernelGGL(class_count_kernel<uint32_t>, grid, blk, 0, st, (const uint32_t*)labels, n, n_classes, (u64*)count);
  SPG_LAUNCH_CHECK();
  return 0;
}
