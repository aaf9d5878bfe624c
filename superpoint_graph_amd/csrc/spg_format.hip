// Result text on the device: numbers to lines, the mirror image of spg_text.hip.  A table of up to
// SPG_TEXT_MAX_COLS columns over n rows becomes the bytes of n lines, fields joined by one space, every line ended by '\n' -- what
// numpy.savetxt writes with fmt='%d' (the label file of the reference's partition/write_Semantic3d.py) and, per record, with
// '%.18g' (plyfile's text writer behind every *2ply function of partition/provider.py).
//
// Two phases, because the byte count sizes the output:
//   spg_format_measure   one row per lane: the length of every field, summed; one rocPRIM exclusive scan -> row_start [n + 1]
//   spg_format_write     one row per lane again: every field is formatted into three 64-bit registers (at most 24 bytes), its
//                        bytes go through an 8-byte word that is stored whole where it lies inside the row, byte by byte at
//                        the row's two ends (the neighbouring lanes own the rest of those words)
// Both phases run the SAME field formatter, so a row's measured length is the number of bytes it writes.
//
// The float32 field ('%.18g' of the exactly widened value) uses integer arithmetic only: the 24-bit significand is placed in a
// fixed-point number of 4 integer and 5 fraction words of 32 bits, the integer words give groups of nine digits by division by
// 10^9, the fraction words by multiplication with 10^9; the groups are fed, most significant first, into a 19-digit
// accumulator plus a sticky flag, and the 19th digit and the flag round the 18 in front of it, ties to even.
//
// Safety:
//   * every loop has a compile-time trip bound (digit groups, words, bytes of a field, columns);
//   * no loop waits on another workgroup, there is no atomic and no flag;
//   * a column is read at row r < n_rows only; every store address is formed from an offset that was compared with
//     row_start[r + 1] and with the caller's capacity first (FormatSink::flush), so a row_start that does not belong to the
//     table truncates rows and never writes out of range;
//   * a capacity below the total is refused on the host before any launch: nothing is written.
#include <climits>
#include <cstdint>
#include <cstring>

#include "../../include/spg_hip.h"
#include "spg_part.h"

namespace {

constexpr int FMT_BLOCK = 256;
constexpr long FMT_MAX_ROWS = 1L << 36;
constexpr int FMT_MAX_FIELD = 24;      // bytes of the longest field: -d.ddddddddddddddddde-XX and -0.000dddddddddddddddddd

typedef uint8_t u8;
typedef uint32_t u32;

constexpr u32 E9 = 1000000000u;

constexpr u64 kFmtPow10[19] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull,
                                  10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull,
                                  1000000000000000ull, 10000000000000000ull, 100000000000000000ull, 1000000000000000000ull};

// the columns of a table: a kernel argument, read with uniform indices
struct FormatCols {
  int n_cols;
  u64 kinds;      // nibble c = the SPG_FORMAT_* of column c
  const void* ptr[SPG_TEXT_MAX_COLS];
  long stride[SPG_TEXT_MAX_COLS];      // in bytes
};

// ---- one field: at most FMT_MAX_FIELD bytes in three registers (selects, not an array: an index by k would live in scratch) ----
struct Field {
  u64 b0, b1, b2;
  int k;
  __host__ __device__ __forceinline__ void push(unsigned c) {
    const u64 v = (u64)c << ((k & 7) * 8);
    if (k < 8) b0 |= v;
    else if (k < 16) b1 |= v;
    else b2 |= v;
    ++k;
  }
};

// digit i (0 = the most significant) of a group of nine
template <int I>
__host__ __device__ __forceinline__ unsigned group_digit(u32 g) {
  constexpr u32 P[9] = {100000000u, 10000000u, 1000000u, 100000u, 10000u, 1000u, 100u, 10u, 1u};
  return '0' + (g / P[I]) % 10u;
}

// the decimal digits of g, 1 <= g < 10^9
__host__ __device__ __forceinline__ int group_length(u32 g) {
  return 1 + (g >= 10u) + (g >= 100u) + (g >= 1000u) + (g >= 10000u) + (g >= 100000u) + (g >= 1000000u) + (g >= 10000000u) +
         (g >= 100000000u);
}

// the trailing zeros of g, 1 <= g < 10^9 (once the last digit is not zero it stays so: no flag)
__host__ __device__ __forceinline__ int group_trailing_zeros(u32 g) {
  int t = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u32 q = g / 10u;
    const bool z = q * 10u == g;
    g = z ? q : g;
    t += z;
  }
  return t;
}

// '%d' of (-)mag
__host__ __device__ __forceinline__ void format_int(Field& f, bool neg, u64 mag) {
  if (neg) f.push('-');
  u32 top, hi, lo;      // mag = top * 10^18 + hi * 10^9 + lo
  if ((mag >> 32) == 0) {
    top = 0u; hi = (u32)mag / E9; lo = (u32)mag - hi * E9;
  } else {
    const u64 q18 = mag / 1000000000000000000ull, rest = mag - q18 * 1000000000000000000ull;
    top = (u32)q18; hi = (u32)(rest / E9); lo = (u32)(rest - (u64)hi * E9);
  }
  bool started = false;
  if (top >= 10u) { f.push('0' + top / 10u); started = true; }
  if (started || top != 0u) { f.push('0' + top % 10u); started = true; }
#define SPG_FMT_DIGIT(G, I, LAST)                         \
  {                                                       \
    const unsigned d = group_digit<I>(G);                 \
    if (started || d != '0' || (LAST)) { f.push(d); started = true; } \
  }
  if (started || hi != 0u) {
    SPG_FMT_DIGIT(hi, 0, false) SPG_FMT_DIGIT(hi, 1, false) SPG_FMT_DIGIT(hi, 2, false) SPG_FMT_DIGIT(hi, 3, false) SPG_FMT_DIGIT(hi, 4, false)
    SPG_FMT_DIGIT(hi, 5, false) SPG_FMT_DIGIT(hi, 6, false) SPG_FMT_DIGIT(hi, 7, false) SPG_FMT_DIGIT(hi, 8, false)
  }
  SPG_FMT_DIGIT(lo, 0, false) SPG_FMT_DIGIT(lo, 1, false) SPG_FMT_DIGIT(lo, 2, false) SPG_FMT_DIGIT(lo, 3, false) SPG_FMT_DIGIT(lo, 4, false)
  SPG_FMT_DIGIT(lo, 5, false) SPG_FMT_DIGIT(lo, 6, false) SPG_FMT_DIGIT(lo, 7, false) SPG_FMT_DIGIT(lo, 8, true)
#undef SPG_FMT_DIGIT
}

// The 19-digit accumulator the groups of nine are fed into, most significant first.
struct Digits {
  u64 acc;      // the first nd significant digits
  int nd, X;    // X: the decimal exponent of the first digit
  bool sticky;  // a digit behind the 19th is not zero
  // low_exp: the decimal exponent of the group's last digit
  __host__ __device__ __forceinline__ void feed(u32 g, int low_exp) {
    if (nd == 0) {
      if (g == 0u) return;
      const int L = group_length(g);
      acc = g; nd = L; X = low_exp + L - 1;
    } else if (nd <= 10) {
      acc = acc * E9 + g; nd += 9;      // at most 19 digits: below 2^64
    } else if (nd < 19) {
      const int need = 19 - nd;         // 1 ... 8
      const u32 p = (u32)kFmtPow10[9 - need], hi = g / p;
      acc = acc * kFmtPow10[need] + hi;
      sticky |= g != hi * p;
      nd = 19;
    } else {
      sticky |= g != 0u;
    }
  }
};

// m * 2^e, 1 <= m < 2^24, -149 <= e <= 104 -> its 18 significant digits q (10^17 <= q < 10^18, correctly rounded, ties to even)
// and the decimal exponent X of the first of them
__host__ __device__ __forceinline__ void f32_decimal(u32 m, int e, u64* q_out, int* X_out) {
  // fixed point: w[0..4] the fraction (w[4] in front), w[5..8] the integer part; bit 0 of m is bit s of the 288
  const int s = e + 160;      // 11 ... 264
  u32 w[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int d = s - 32 * j;
    w[j] = (d > -32 && d <= 32) ? (u32)((((u64)m) << 32) >> (32 - d)) : 0u;
  }
  Digits D = {0ull, 0, 0, false};
  // the integer part: groups of nine from the low end, fed from the high end
  if ((w[6] | w[7] | w[8]) != 0u) {
    u32 ig[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      u64 rem = 0ull;
#pragma unroll
      for (int j = 8; j >= 5; --j) {
        const u64 cur = rem << 32 | w[j];
        const u64 q = cur / E9;
        w[j] = (u32)q;
        rem = cur - q * E9;
      }
      ig[k] = (u32)rem;
    }
#pragma unroll
    for (int k = 4; k >= 0; --k) D.feed(ig[k], 9 * k);
  } else if (w[5] != 0u) {
    const u32 g1 = w[5] / E9;
    D.feed(g1, 9);
    D.feed(w[5] - g1 * E9, 0);
  }
  // the fraction: 8 groups reach decimal place 72; the first digit of 2^-149 is at place 45 and 45 + 18 <= 72
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    if (D.nd < 19 && (w[0] | w[1] | w[2] | w[3] | w[4]) != 0u) {
      u64 carry = 0ull;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const u64 cur = (u64)w[j] * E9 + carry;
        w[j] = (u32)cur;
        carry = cur >> 32;
      }
      D.feed((u32)carry, -9 * g - 9);
    }
  }
  D.sticky |= (w[0] | w[1] | w[2] | w[3] | w[4]) != 0u;
  u64 q;
  if (D.nd == 19) {
    q = D.acc / 10ull;
    const unsigned d = (unsigned)(D.acc - q * 10ull);
    if (d > 5u || (d == 5u && (D.sticky || (q & 1ull)))) ++q;
    if (q == kFmtPow10[18]) { q = kFmtPow10[17]; ++D.X; }
  } else {
    q = D.acc * kFmtPow10[18 - D.nd];      // the value has fewer digits: exact
  }
  *q_out = q;
  *X_out = D.X;
}

// Python's '%.18g' % float(v)
__host__ __device__ __forceinline__ void format_f32(Field& f, u32 bits) {
  const u32 ex = bits >> 23 & 255u, frac = bits & 0x7fffffu;
  const bool neg = bits >> 31;
  if (ex == 255u) {
    if (frac != 0u) { f.push('n'); f.push('a'); f.push('n'); return; }
    if (neg) f.push('-');
    f.push('i'); f.push('n'); f.push('f');
    return;
  }
  if (neg) f.push('-');
  const u32 m = ex != 0u ? frac | 0x800000u : frac;
  if (m == 0u) { f.push('0'); return; }
  u64 q;
  int X;
  f32_decimal(m, (ex != 0u ? (int)ex : 1) - 150, &q, &X);
  const u32 hi = (u32)(q / E9), lo = (u32)(q - (u64)hi * E9);
  const int P = lo == 0u ? 9 - group_trailing_zeros(hi) : 18 - group_trailing_zeros(lo);      // digits once trailing zeros are gone
  const bool fixed = X >= -4 && X < 18;
  int nd = P, dot_at = 0;
  if (fixed && X < 0) {
    f.push('0'); f.push('.');
#pragma unroll
    for (int z = 0; z < 3; ++z)
      if (z < -X - 1) f.push('0');
    dot_at = -1;
  } else if (fixed) {
    nd = P > X + 1 ? P : X + 1;
    dot_at = X;
  }
#define SPG_FMT_DIGIT(G, I, AT)                      \
  if ((AT) < nd) {                                   \
    f.push(group_digit<I>(G));                       \
    if ((AT) == dot_at && (AT) + 1 < nd) f.push('.'); \
  }
  SPG_FMT_DIGIT(hi, 0, 0) SPG_FMT_DIGIT(hi, 1, 1) SPG_FMT_DIGIT(hi, 2, 2) SPG_FMT_DIGIT(hi, 3, 3) SPG_FMT_DIGIT(hi, 4, 4)
  SPG_FMT_DIGIT(hi, 5, 5) SPG_FMT_DIGIT(hi, 6, 6) SPG_FMT_DIGIT(hi, 7, 7) SPG_FMT_DIGIT(hi, 8, 8)
  SPG_FMT_DIGIT(lo, 0, 9) SPG_FMT_DIGIT(lo, 1, 10) SPG_FMT_DIGIT(lo, 2, 11) SPG_FMT_DIGIT(lo, 3, 12) SPG_FMT_DIGIT(lo, 4, 13)
  SPG_FMT_DIGIT(lo, 5, 14) SPG_FMT_DIGIT(lo, 6, 15) SPG_FMT_DIGIT(lo, 7, 16) SPG_FMT_DIGIT(lo, 8, 17)
#undef SPG_FMT_DIGIT
  if (!fixed) {
    const unsigned a = (unsigned)(X < 0 ? -X : X);      // at most 45
    f.push('e'); f.push(X < 0 ? '-' : '+'); f.push('0' + a / 10u); f.push('0' + a % 10u);
  }
}

// the value at p as a field
__host__ __device__ __forceinline__ Field format_value(int kind, const char* p) {
  Field f = {0ull, 0ull, 0ull, 0};
  if (kind == SPG_FORMAT_F32) {
    format_f32(f, *(const u32*)p);
  } else {
    bool neg = false;
    u64 mag;
    if (kind == SPG_FORMAT_U8) mag = *(const u8*)p;
    else if (kind == SPG_FORMAT_U32) mag = *(const u32*)p;
    else {
      const int64_t v = kind == SPG_FORMAT_I32 ? (int64_t)*(const int32_t*)p : *(const int64_t*)p;
      neg = v < 0;
      mag = neg ? 0ull - (u64)v : (u64)v;
    }
    format_int(f, neg, mag);
  }
  return f;
}

// field c of row r
__device__ __forceinline__ Field format_field(const FormatCols& cols, int c, long r) {
  return format_value((int)(cols.kinds >> (4 * c) & 15u), (const char*)cols.ptr[c] + r * cols.stride[c]);
}

__global__ __launch_bounds__(FMT_BLOCK) void format_measure_kernel(FormatCols cols, long n, int* __restrict__ len) {
  const long r = (long)blockIdx.x * FMT_BLOCK + threadIdx.x;
  if (r >= n) return;
  int total = 0;
#pragma unroll 1
  for (int c = 0; c < SPG_TEXT_MAX_COLS; ++c) {
    if (c >= cols.n_cols) break;
    total += format_field(cols, c, r).k + 1;      // the separator or the '\n'
  }
  len[r] = total;
}

// The bytes of a row on their way out: collected in the 8-byte word they fall into (out is 8-byte aligned).  lo / hi: the row
// owns [lo, hi), hi already cut at the capacity.
struct FormatSink {
  u8* out;
  long pos, lo, hi;
  u64 word;
  // the bytes [base, pos) of the word that starts at base
  __device__ __forceinline__ void flush(long base) {
    if (base >= lo && base + 8 <= hi && pos == base + 8) {
      *(u64*)(out + base) = word;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const long p = base + j;
        if (p >= lo && p < pos && p < hi) out[p] = (u8)(word >> (8 * j));
      }
    }
    word = 0ull;
  }
  __device__ __forceinline__ void put(unsigned c) {
    word |= (u64)c << ((pos & 7) * 8);
    ++pos;
    if ((pos & 7) == 0) flush(pos - 8);
  }
  __device__ __forceinline__ void finish() {
    if ((pos & 7) != 0) flush(pos & ~7L);
  }
};

__global__ __launch_bounds__(FMT_BLOCK) void format_write_kernel(FormatCols cols, long n, const int64_t* __restrict__ row_start,
                                                                 u8* __restrict__ out, long capacity) {
  const long r = (long)blockIdx.x * FMT_BLOCK + threadIdx.x;
  if (r >= n) return;
  const long lo = row_start[r], next = row_start[r + 1];
  if (lo < 0 || next < lo) return;      // (not the row_start of a table)
  FormatSink sink = {out, lo, lo, next < capacity ? next : capacity, 0ull};
#pragma unroll 1
  for (int c = 0; c < SPG_TEXT_MAX_COLS; ++c) {
    if (c >= cols.n_cols) break;
    Field f = format_field(cols, c, r);
#pragma unroll 1
    for (int j = 0; j < FMT_MAX_FIELD; ++j) {
      if (j >= f.k) break;
      sink.put((unsigned)(f.b0 & 255ull));
      f.b0 = f.b0 >> 8 | f.b1 << 56;
      f.b1 = f.b1 >> 8 | f.b2 << 56;
      f.b2 >>= 8;
    }
    sink.put(c + 1 == cols.n_cols ? '\n' : ' ');
  }
  sink.finish();
}

// ---- error2ply's colours (partition/provider.py:73-98): colorsys in float64, operation by operation ----
__global__ __launch_bounds__(FMT_BLOCK) void error_colour_kernel(const u8* __restrict__ rgb, const int64_t* __restrict__ labels,
                                                                 const int64_t* __restrict__ prediction, long n, u8* __restrict__ out) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * FMT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double r = (double)rgb[3 * i] / 255.0, g = (double)rgb[3 * i + 1] / 255.0, b = (double)rgb[3 * i + 2] / 255.0;
  // rgb_to_hsv: the hue is replaced, saturation and value remain
  const double rg = r > g ? r : g, maxc = rg > b ? rg : b;
  const double rg_ = r < g ? r : g, minc = rg_ < b ? rg_ : b;
  double v = maxc, s = 0.0;
  if (minc != maxc) s = (maxc - minc) / maxc;
  const int64_t label = labels[i];
  const double h = (label == prediction[i] || label == 0) ? 0.333333 : 0.0;
  const double s3 = s + 0.3, v1 = v + 0.1;
  s = s3 < 1.0 ? s3 : 1.0;
  v = v1 < 1.0 ? v1 : 1.0;
  // hsv_to_rgb (s >= 0.3: its grey branch is never taken; h * 6 < 2: sectors 0 and 1 only)
  const double h6 = h * 6.0;
  const int sector = (int)h6;
  const double f = h6 - (double)sector;
  const double p = v * (1.0 - s);
  const double q = v * (1.0 - s * f);
  const double t = v * (1.0 - s * (1.0 - f));
  const double R = sector == 0 ? v : q, G = sector == 0 ? t : v;
  out[3 * i] = (u8)(int)(R * 255.0);
  out[3 * i + 1] = (u8)(int)(G * 255.0);
  out[3 * i + 2] = (u8)(int)(p * 255.0);
}

struct FormatWs {
  int* len;      // [n + 1], the last one zero
  void* tmp;
  size_t tmp_bytes;
  FormatWs(Carve& w, long n) {
    len = w.take_n<int>((size_t)n + 1);
    tmp_bytes = exclusive_scan_bytes<int64_t>(n + 1, (int*)nullptr);
    tmp = w.take(tmp_bytes);
  }
};

constexpr int kKindBytes[SPG_FORMAT_KINDS] = {1, 4, 4, 8, 4};

// the host's description of the table, checked -> the kernel argument
int format_cols(const void* const* columns, const int* kinds, const long* strides, int n_cols, long n_rows, FormatCols* cols) {
  SPG_CHECK_ARG(n_cols >= 1 && n_cols <= SPG_TEXT_MAX_COLS, "1 <= n_cols <= SPG_TEXT_MAX_COLS");
  SPG_CHECK_ARG(n_rows >= 0 && n_rows <= FMT_MAX_ROWS && columns && kinds && strides, "bad argument");
  *cols = FormatCols{};
  cols->n_cols = n_cols;
  for (int c = 0; c < n_cols; ++c) {
    SPG_CHECK_ARG(kinds[c] >= 0 && kinds[c] < SPG_FORMAT_KINDS, "a column kind outside SPG_FORMAT_*");
    const int bytes = kKindBytes[kinds[c]];
    SPG_CHECK_ARG(n_rows == 0 || columns[c], "null column");
    SPG_CHECK_ARG(strides[c] >= 0 && strides[c] <= (LONG_MAX >> 4) / std::max<long>(n_rows, 1), "a column stride that is negative or overflows");
    SPG_CHECK_ARG(((uintptr_t)columns[c] & (uintptr_t)(bytes - 1)) == 0, "a column that is not aligned to its element");
    cols->kinds |= (u64)kinds[c] << (4 * c);
    cols->ptr[c] = columns[c];
    cols->stride[c] = strides[c] * bytes;
  }
  return 0;
}

}  // namespace

extern "C" size_t spg_format_workspace_bytes(long n_rows, int n_cols) {
  if (n_rows < 0 || n_rows > FMT_MAX_ROWS || n_cols < 1 || n_cols > SPG_TEXT_MAX_COLS) return 0;
  Carve w;
  FormatWs l(w, n_rows);
  return w.used();
}

extern "C" int spg_format_measure(const void* const* columns, const int* kinds, const long* strides, int n_cols, long n_rows,
                                  int64_t* row_start, void* workspace, size_t workspace_bytes, void* stream) {
  FormatCols cols;
  SPG_TRY(format_cols(columns, kinds, strides, n_cols, n_rows, &cols));
  SPG_CHECK_ARG(row_start && workspace, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  Carve w(workspace, workspace_bytes);
  FormatWs l(w, n_rows);
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_format_workspace_bytes(n_rows, n_cols))");
  SPG_RP(hipMemsetAsync(l.len + n_rows, 0, sizeof(int), st));
  if (n_rows > 0) {
    hipLaunchKernelGGL(format_measure_kernel, dim3((unsigned)spg_cdiv(n_rows, FMT_BLOCK)), dim3(FMT_BLOCK), 0, st, cols, n_rows, l.len);
    SPG_LAUNCH_CHECK();
  }
  size_t b = l.tmp_bytes;
  SPG_RP(rocprim::exclusive_scan(l.tmp, b, l.len, row_start, (int64_t)0, (size_t)(n_rows + 1), rocprim::plus<int64_t>(), st));
  return 0;
}

extern "C" int spg_format_write(const void* const* columns, const int* kinds, const long* strides, int n_cols, long n_rows,
                                const int64_t* row_start, long total_bytes, uint8_t* out, long capacity, void* stream) {
  FormatCols cols;
  SPG_TRY(format_cols(columns, kinds, strides, n_cols, n_rows, &cols));
  SPG_CHECK_ARG(row_start && total_bytes >= 0 && capacity >= 0 && (out || capacity == 0), "bad argument");
  SPG_CHECK_ARG(capacity >= total_bytes, "the output buffer is smaller than the table's text (row_start[n_rows] bytes)");
  SPG_CHECK_ARG(((uintptr_t)out & 7) == 0, "out must be 8-byte aligned");
  if (n_rows == 0 || total_bytes == 0) return 0;
  hipLaunchKernelGGL(format_write_kernel, dim3((unsigned)spg_cdiv(n_rows, FMT_BLOCK)), dim3(FMT_BLOCK), 0, (hipStream_t)stream, cols, n_rows,
                     row_start, out, capacity);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_format_debug_field(int kind, const void* value, char* out) {
  if (kind < 0 || kind >= SPG_FORMAT_KINDS || !value || !out) return -1;
  Field f = format_value(kind, (const char*)value);
  for (int j = 0; j < f.k; ++j) out[j] = (char)((j < 8 ? f.b0 : j < 16 ? f.b1 : f.b2) >> (8 * (j & 7)));
  return f.k;
}

extern "C" int spg_error_colours(const uint8_t* rgb, const int64_t* labels, const int64_t* prediction, long n, uint8_t* out, void* stream) {
  SPG_CHECK_ARG(n >= 0 && n <= FMT_MAX_ROWS && (n == 0 || (rgb && labels && prediction && out)), "bad argument");
  if (n == 0) return 0;
  hipLaunchKernelGGL(error_colour_kernel, dim3((unsigned)spg_cdiv(n, FMT_BLOCK)), dim3(FMT_BLOCK), 0, (hipStream_t)stream, rgb, labels,
                     prediction, n, out);
  SPG_LAUNCH_CHECK();
  return 0;
}
