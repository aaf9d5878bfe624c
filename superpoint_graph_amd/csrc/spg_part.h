// Shared plumbing of the partition-pipeline units (spg_spgraph, spg_knn, spg_edgeloss, spg_parteval, spg_tiles): the workspace
// convention, the rocPRIM scratch-size queries and the float helpers whose rounding the reference fixes.
//
// Workspace convention: every entry point that takes a workspace describes it ONCE, as a struct whose
// constructor takes a Carve and the dimensions and performs the take() calls.  spg_*_workspace_bytes runs that constructor on a
// sizing Carve and returns used(); the entry point runs it on the caller's buffer and checks ok before its first launch.  The
// size is what the layout consumes -- there is no slack constant to absorb a forgotten buffer.
//
// The first section (align256, bits_of, Carve) is plain C++ and compiles without HIP; the rest needs hipcc.
#pragma once
#include <algorithm>
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
#endif  // __HIPCC__
