// Shared plumbing of the partition-pipeline units (spg_spgraph, spg_knn, spg_edgeloss, spg_parteval, spg_tiles, spg_structure,
// spg_plane, spg_parsed): the workspace convention, the rocPRIM scratch-size queries, the float helpers whose rounding the
// reference fixes, and the fixed-order reduction.
//
// Workspace convention: every entry point that takes a workspace describes it ONCE, as a struct whose
// constructor takes a Carve and the dimensions and performs the take() calls.  spg_*_workspace_bytes runs that constructor on a
// sizing Carve and returns used(); the entry point runs it on the caller's buffer and checks ok before its first launch.  The
// size is what the layout consumes -- there is no slack constant to absorb a forgotten buffer.
//
// The first section (align256, bits_of, Carve) is plain C++ and compiles without HIP; the rest needs hipcc.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int bits_of(unsigned long v) { int b = 1; while (b < 64 && (v >> b) != 0) ++b; return b; }

// Bump allocator over a caller's workspace in 256-byte steps.  Carve() only measures: it hands out null pointers, never fails and
// adds up in used() exactly what Carve(ws, bytes) would consume.  The position is an offset; a pointer is formed from a real base only.
struct Carve {
  char* base = nullptr;
  size_t size = 0, off = 0;
  bool sizing = true, ok = true;
  Carve() {}
  Carve(void* ws, size_t bytes) : base((char*)ws), size(bytes), sizing(false), ok(ws != nullptr) {}
  void* take(size_t bytes) {
    bytes = align256(bytes);
    if (!sizing && (!ok || bytes > size - off)) { ok = false; return nullptr; }
    void* r = sizing ? nullptr : base + off;
    off += bytes;
    return r;
  }
  template <typename T>
  T* take_n(size_t count) { return (T*)take(count * sizeof(T)); }
  size_t used() const { return off; }
  size_t left() const { return sizing ? 0 : size - off; }
};

#ifdef __HIPCC__
#include <rocprim/rocprim.hpp>

#include "spg_common.h"

typedef unsigned long long u64;

// a rocPRIM / HIP call that returns hipError_t: record and return on failure
#define SPG_RP(expr)                                                                      \
  do {                                                                                    \
    hipError_t e__ = (expr);                                                              \
    if (e__ != hipSuccess) {                                                              \
      spg_set_error("%s:%d: %s: %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__));  \
      return (int)e__;                                                                    \
    }                                                                                     \
  } while (0)

// ---- rocPRIM scratch sizes, named after the call they size; element types and bit ranges are part of the query ----
template <typename K, typename V>
size_t radix_sort_pairs_bytes(long n, unsigned begin_bit, unsigned end_bit) {
  size_t b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, b, (K*)nullptr, (K*)nullptr, (V*)nullptr, (V*)nullptr, (size_t)n, begin_bit, end_bit, (hipStream_t)0);
  return b;
}
template <typename K>
size_t radix_sort_keys_bytes(long n, unsigned begin_bit, unsigned end_bit) {
  size_t b = 0;
  (void)rocprim::radix_sort_keys(nullptr, b, (K*)nullptr, (K*)nullptr, (size_t)n, begin_bit, end_bit, (hipStream_t)0);
  return b;
}
template <typename K, typename C>      // keys K, run lengths C, run count unsigned
size_t run_length_encode_bytes(long n) {
  size_t b = 0;
  (void)rocprim::run_length_encode(nullptr, b, (K*)nullptr, (unsigned)n, (K*)nullptr, (C*)nullptr, (unsigned*)nullptr, (hipStream_t)0);
  return b;
}
template <typename T, typename In>
size_t exclusive_scan_bytes(long n, In in) {
  size_t b = 0;
  (void)rocprim::exclusive_scan(nullptr, b, in, (T*)nullptr, (T)0, (size_t)n, rocprim::plus<T>(), (hipStream_t)0);
  return b;
}
template <typename T>
size_t exclusive_scan_bytes(long n) { return exclusive_scan_bytes<T>(n, (T*)nullptr); }
template <typename T, typename F>      // values T, flags F, selected count T
size_t select_bytes(long n) {
  size_t b = 0;
  (void)rocprim::select(nullptr, b, (T*)nullptr, (F*)nullptr, (T*)nullptr, (T*)nullptr, (size_t)n, (hipStream_t)0);
  return b;
}

// ---- float -> unsigned with the same order; -0.0 and +0.0 are one value (np.unique compares with ==) ----
__device__ __forceinline__ unsigned ordered_bits(float f) {
  unsigned b = __float_as_uint(f);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float from_ordered(unsigned b) { return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b); }

// correctly rounded float32 square root, as np.sqrt of a float32 array returns it.  (__fsqrt_rn is NOT that here: without
// OCML_BASIC_ROUNDED_OPERATIONS the HIP headers map it to the native instruction, good to one ulp.)  The float64 root is correctly
// rounded and 53 >= 2 * 24 + 2 bits, so rounding it once more to float32 cannot differ from rounding the exact root.
__device__ __forceinline__ float sqrt_rn_f32(float x) { return (float)sqrt((double)x); }

// dx*dx + dy*dy (+ dz*dz) in float32, every product and every sum rounded on its own, added left to right -- what numpy does
// with a float32 array.  (__fmul_rn / __fadd_rn do NOT guarantee that here: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers
// define them as plain * and +, which the compiler contracts into fused multiply-adds.)
__device__ __forceinline__ float sumsq2_rn_f32(float dx, float dy) {
#pragma clang fp contract(off)
  const float xx = dx * dx, yy = dy * dy;
  return xx + yy;
}
__device__ __forceinline__ float sumsq3_rn_f32(float dx, float dy, float dz) {
#pragma clang fp contract(off)
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float xy = xx + yy;
  return xy + zz;
}

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ---- the fixed-order reduction ----
// Workgroups of PART_BLOCK threads, at most PART_MAX_BLOCKS of them with a grid stride beyond; inside a workgroup the xor
// butterfly 32, 16, ..., 1 in every wave, then waves 0, 1, 2, 3 in that order through LDS.  The grid depends on n alone, there is no
// floating-point atomic and no waiting between workgroups: the same input gives the same bits.
constexpr int PART_BLOCK = 256;
constexpr int PART_WAVES = PART_BLOCK / 64;
constexpr int PART_MAX_BLOCKS = 1024;
inline int part_reduce_blocks(long n) { return std::min(spg_cdiv(std::max<long>(n, 1), PART_BLOCK), PART_MAX_BLOCKS); }

enum { PART_MIN, PART_MAX, PART_SUM };
template <int OP> struct PartAll { static constexpr int op(int) { return OP; } };      // every component by the same operation

__device__ __forceinline__ float part_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double part_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float part_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double part_max(double a, double b) { return fmax(a, b); }
// (op is an argument so that a loop over components can pass Ops::op(c); it is a constant at every call and the branch folds away)
template <typename T>
__device__ __forceinline__ T part_combine(int op, T a, T b) { return op == PART_MIN ? part_min(a, b) : op == PART_MAX ? part_max(a, b) : a + b; }
template <typename T>
__device__ __forceinline__ T part_identity(int op) { return op == PART_MIN ? (T)INFINITY : op == PART_MAX ? (T)-INFINITY : (T)0; }

// the wave's value in every lane (a + b and b + a are one value, so all lanes hold the same bits)
template <typename T>
__device__ __forceinline__ T wave_reduce(int op, T v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = part_combine(op, v, __shfl_xor(v, off, 64));
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce(PART_SUM, v); }

// the workgroup's K values in every thread; component c combines by Ops::op(c).  lds: [PART_WAVES][K], free on entry; one barrier.
template <typename Ops, typename T, int K>
__device__ __forceinline__ void block_reduce(T (&v)[K], T (*lds)[K]) {
#pragma unroll
  for (int c = 0; c < K; ++c) {
    v[c] = wave_reduce(Ops::op(c), v[c]);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6][c] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < K; ++c) {
    v[c] = lds[0][c];
#pragma unroll
    for (int w = 1; w < PART_WAVES; ++w) v[c] = part_combine(Ops::op(c), v[c], lds[w][c]);
  }
}

// block-wide OR of `bad`, then thread 0 sets `bits` in the error word.  Every thread of the workgroup calls it.
__device__ __forceinline__ void block_report(int bad, int32_t* err, int bits) {
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0 && bad) atomicOr(err, bits);
}

// The two-phase pass over the points of a scene.  A pass P is a small struct passed by value:
//   typedef T; static constexpr int K; static constexpr int op(int c);        K values of type T, component c combined by op(c)
//   __device__ void point(const float* xyz, long i, T (&v)[K], int& bad) const   what point i contributes; bad |= a coordinate is not finite
//   __device__ void write(const T (&v)[K], long n) const                         thread 0 of the final workgroup: the results
// part_partial_kernel leaves one row of K partials per workgroup, part_final_kernel is ONE workgroup over the rows in the same shape.
template <typename P>
__global__ __launch_bounds__(PART_BLOCK) void part_partial_kernel(P p, const float* __restrict__ xyz, long n,
                                                                  typename P::T* __restrict__ partials, int32_t* __restrict__ err) {
  typedef typename P::T T;
  __shared__ T lds[PART_WAVES][P::K];
  T v[P::K];
#pragma unroll
  for (int c = 0; c < P::K; ++c) v[c] = part_identity<T>(P::op(c));
  int bad = 0;
  for (long i = (long)blockIdx.x * PART_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * PART_BLOCK) p.point(xyz, i, v, bad);
  if (err != nullptr) block_report(bad, err, 1);
  block_reduce<P>(v, lds);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int c = 0; c < P::K; ++c) partials[P::K * (long)blockIdx.x + c] = v[c];
}

template <typename P>
__global__ __launch_bounds__(PART_BLOCK) void part_final_kernel(P p, const typename P::T* __restrict__ partials, int nb, long n) {
  typedef typename P::T T;
  __shared__ T lds[PART_WAVES][P::K];
  T v[P::K];
#pragma unroll
  for (int c = 0; c < P::K; ++c) v[c] = part_identity<T>(P::op(c));
  for (int b = threadIdx.x; b < nb; b += PART_BLOCK) {
#pragma unroll
    for (int c = 0; c < P::K; ++c) v[c] = part_combine(P::op(c), v[c], partials[P::K * (long)b + c]);
  }
  block_reduce<P>(v, lds);
  if (threadIdx.x == 0) p.write(v, n);
}

// err: the error word whose bit 0 reports a coordinate that is not finite, or null for a pass that does not check
template <typename P>
int part_reduce(const P& p, const float* xyz, long n, typename P::T* partials, int blocks, int32_t* err, hipStream_t st) {
  hipLaunchKernelGGL(part_partial_kernel<P>, dim3(blocks), dim3(PART_BLOCK), 0, st, p, xyz, n, partials, err);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(part_final_kernel<P>, dim3(1), dim3(PART_BLOCK), 0, st, p, (const typename P::T*)partials, blocks, n);
  SPG_LAUNCH_CHECK();
  return 0;
}

// per-axis minimum / maximum of xyz [n, 3] into mm[0..2] / mm[3..5] as ordered bits (integer atomics: the order does not matter);
// any grid of whole waves.  -> a coordinate this thread read is not finite
__device__ __forceinline__ bool axis_minmax(const float* __restrict__ xyz, long n, unsigned* __restrict__ mm) {
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    for (int d = 0; d < 3; ++d) {
      const float v = xyz[3 * i + d];
      bad |= !finite_f32(v);
      lo[d] = fminf(lo[d], v); hi[d] = fmaxf(hi[d], v);
    }
  for (int d = 0; d < 3; ++d) {
    lo[d] = wave_reduce(PART_MIN, lo[d]); hi[d] = wave_reduce(PART_MAX, hi[d]);
    if ((threadIdx.x & 63) == 0) { atomicMin(&mm[d], ordered_bits(lo[d])); atomicMax(&mm[3 + d], ordered_bits(hi[d])); }
  }
  return bad;
}
#endif  // __HIPCC__
