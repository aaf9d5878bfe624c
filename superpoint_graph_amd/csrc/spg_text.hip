// Raw cloud text on the device: the `x y z i r g b` lines of Semantic3D and the `x y z r g b` lines of
// S3DIS, which the reference reads with pandas.read_csv (partition/provider.py:185-217, :250-303, :637-679).
//
// Two phases, because the number of lines sizes the outputs:
//   spg_text_index   starts of the non-blank lines counted per 4 KiB tile (16-byte loads), one rocPRIM scan over the tile counts
//                    and one rocPRIM maximum over the tiles' last '\n', then head = {lines, bytes consumed} on the device
//   spg_text_lines   the same tiles again: the start offsets, placed through the scanned tile offsets
//   spg_text_parse   one line per lane, the bytes read from global memory (lanes of a wave read neighbouring lines, the
//                    cache lines are shared).  Staging a workgroup's span in LDS first measured 3 % slower
//                    (profiles/cloud_text_variants.txt) and was removed.
//
// Safety: every byte address is formed from an offset that was compared with n_bytes first; the loop over a line's bytes ends at
// its terminator, at n_bytes or after TEXT_MAX_LINE bytes, whichever comes first.  A buffer outside the grammar gives an error
// record, never a read out of range.
#include <climits>
#include <cstdint>
#include <cstring>

#include "../../include/spg_hip.h"
#include "spg_part.h"

namespace {

constexpr int TEXT_BLOCK = 256;
constexpr int TEXT_INDEX_TILE = TEXT_BLOCK * 16;      // bytes per workgroup of the index kernels: one 16-byte load per lane
constexpr int TEXT_MAX_LINE = SPG_TEXT_MAX_LINE;      // bytes of a line in front of its terminator
constexpr int TEXT_MAX_DIGITS = 15, TEXT_MAX_FRACTION = 22;
constexpr long TEXT_MAX_BYTES = 1L << 40;

typedef uint8_t u8;

// 16 bytes at offset o (a multiple of 16; text is 16-byte aligned), zeros past n
__device__ __forceinline__ uint4 text_load16(const u8* __restrict__ text, long n, long o) {
  if (o + 16 <= n) return *(const uint4*)(text + o);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  u8* b = (u8*)&v;
  for (int j = 0; j < 16; ++j)
    if (o + j < n) b[j] = text[o + j];
  return v;
}

// does a non-blank line start at p?  (p == 0 or the byte in front is '\n'; the line is not empty in front of its terminator)
__device__ __forceinline__ bool text_is_start(const u8* __restrict__ text, long n, long p) {
  if (p >= n || (p > 0 && text[p - 1] != '\n')) return false;
  const u8 c = text[p];
  if (c == '\n') return false;
  return !(c == '\r' && p + 1 < n && text[p + 1] == '\n');
}

// the 16 bytes of this lane: bit j of the result = a non-blank line starts at o + j; *last_nl = 1 + the offset of the last '\n'
// among them, or 0
__device__ __forceinline__ unsigned text_chunk_starts(const u8* __restrict__ text, long n, long o, long* last_nl) {
  *last_nl = 0;
  if (o >= n) return 0u;
  const uint4 v = text_load16(text, n, o);
  const u8* b = (const u8*)&v;
  u8 prev = o > 0 ? text[o - 1] : (u8)'\n';
  const u8 after = o + 16 < n ? text[o + 16] : (u8)0;
  unsigned mask = 0u;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const long p = o + j;
    if (p < n) {
      const u8 c = b[j];
      const u8 next = j < 15 ? b[j + 1] : after;      // zero past n: never '\n'
      if (prev == '\n' && c != '\n' && !(c == '\r' && next == '\n')) mask |= 1u << j;
      if (c == '\n') *last_nl = p + 1;
      prev = c;
    }
  }
  return mask;
}

__global__ __launch_bounds__(TEXT_BLOCK) void text_count_kernel(const u8* __restrict__ text, long n, unsigned* __restrict__ counts,
                                                                u64* __restrict__ tile_nl) {
  __shared__ long lds[PART_WAVES][2];
  const long o = (long)blockIdx.x * TEXT_INDEX_TILE + threadIdx.x * 16;
  long nl;
  const unsigned mask = text_chunk_starts(text, n, o, &nl);
  long v[2] = {(long)__popc(mask), nl};
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    v[0] += __shfl_xor(v[0], off, 64);
    const long w = __shfl_xor(v[1], off, 64);
    v[1] = w > v[1] ? w : v[1];
  }
  if ((threadIdx.x & 63) == 0) { lds[threadIdx.x >> 6][0] = v[0]; lds[threadIdx.x >> 6][1] = v[1]; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  long c = 0, m = 0;
  for (int w = 0; w < PART_WAVES; ++w) { c += lds[w][0]; m = lds[w][1] > m ? lds[w][1] : m; }
  counts[blockIdx.x] = (unsigned)c;
  tile_nl[blockIdx.x] = (u64)m;
}

// head[0] = lines, head[1] = bytes up to and including the last complete line
__global__ void text_head_kernel(const u8* __restrict__ text, long n, int final_block, const int64_t* __restrict__ tile_off, long n_tiles,
                                 const u64* __restrict__ last_nl, int64_t* __restrict__ head) {
  const long after_nl = (long)*last_nl;      // the unfinished tail starts here
  const bool tail = text_is_start(text, n, after_nl);
  head[0] = tile_off[n_tiles] - ((!final_block && tail) ? 1 : 0);
  head[1] = final_block ? n : after_nl;
}

__global__ __launch_bounds__(TEXT_BLOCK) void text_place_kernel(const u8* __restrict__ text, long n, const int64_t* __restrict__ tile_off,
                                                                long n_lines, int64_t* __restrict__ line_start) {
  __shared__ int totals[PART_WAVES];
  const long o = (long)blockIdx.x * TEXT_INDEX_TILE + threadIdx.x * 16;
  long nl;
  const unsigned mask = text_chunk_starts(text, n, o, &nl);
  const int c = __popc(mask), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int w = __shfl_up(inc, off, 64);
    if (lane >= off) inc += w;
  }
  if (lane == 63) totals[wave] = inc;
  __syncthreads();
  long at = tile_off[blockIdx.x] + (inc - c);
  for (int w = 0; w < wave; ++w) at += totals[w];
  for (int j = 0; j < 16; ++j)
    if (mask >> j & 1u) {
      if (at < n_lines) line_start[at] = o + j;      // (the unfinished tail of a block that is not the last is not a line)
      ++at;
    }
}

// ---- one line ----
// the role of every column, 4 bits each (a register, not an array: an index by the running field would put an array in scratch)
struct TextCols {
  int n_cols;
  u64 roles;      // nibble c = 1 + the role of column c: 0 validated and dropped, 1..3 xyz, 4..6 rgb, 7 label
  __host__ __device__ int role(int c) const { return (int)(roles >> (4 * c) & 15u) - 1; }
};

struct TextRow {
  float x, y, z;
  u8 r, g, b, label;
  __device__ __forceinline__ void set(int role, float f, u8 v) {
    if (role == 0) x = f; else if (role == 1) y = f; else if (role == 2) z = f;
    else if (role == 3) r = v; else if (role == 4) g = v; else if (role == 5) b = v; else label = v;
  }
};

__device__ const double kTextPow10[TEXT_MAX_FRACTION + 1] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                                             1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// Parses the line that starts at s; `byte(p)` returns text[p] for s <= p < n.  -> 0 or the SPG_TEXT_ERR_* of the first refusal met
// walking the bytes from the left (a token is judged at its end), *where = its byte offset.
template <typename Byte>
__device__ __forceinline__ int text_parse_line(const Byte& byte, long n, long s, const TextCols& cols, TextRow* row, long* where) {
  int field = 0, n_digit = 0, n_sig = 0, n_frac = 0;
  bool neg = false, dot = false, malformed = false;
  u64 M = 0;
  long tok = s;
  for (long p = s;; ++p) {
    const bool at_end = p >= n;
    unsigned c = at_end ? (unsigned)'\n' : byte(p);
    if (c == '\r' && p + 1 < n && byte(p + 1) == '\n') c = '\n';
    if (c != '\n' && p - s >= TEXT_MAX_LINE) { *where = p; return SPG_TEXT_ERR_LONG; }
    if (c == ' ' || c == '\n') {
      if (p == tok) { *where = p; return SPG_TEXT_ERR_EMPTY; }
      *where = tok;
      if (field >= cols.n_cols) return SPG_TEXT_ERR_FIELDS;
      if (malformed || n_digit == 0 || n_sig > TEXT_MAX_DIGITS || n_frac > TEXT_MAX_FRACTION) return SPG_TEXT_ERR_TOKEN;
      const int role = cols.role(field);
      if (role >= 0) {
        const double v = (double)M / kTextPow10[n_frac];      // M < 10^15 and 10^f, f <= 22, are exact: the correctly rounded double
        const float f = (float)v;
        if (role >= 3 && ((neg && v != 0.0) || v > 255.0 || v != floor(v))) return SPG_TEXT_ERR_RANGE;
        row->set(role, (neg && f != 0.0f) ? -f : f, role >= 3 ? (u8)v : (u8)0);      // zeros are +0.0 whatever their sign
      }
      ++field;
      if (c == '\n') {
        if (field != cols.n_cols) { *where = p; return SPG_TEXT_ERR_FIELDS; }
        return 0;
      }
      tok = p + 1;
      n_digit = n_sig = n_frac = 0; neg = dot = malformed = false; M = 0;
    } else if (c >= '0' && c <= '9') {
      const unsigned d = c - '0';
      ++n_digit;
      if (dot) ++n_frac;
      if (M != 0 || d != 0) {
        if (++n_sig <= TEXT_MAX_DIGITS) M = M * 10 + d;
      }
    } else if (c == '.') {
      if (dot) malformed = true;
      dot = true;
    } else if (c == '+' || c == '-') {
      if (p != tok) malformed = true;
      neg = c == '-';
    } else {
      *where = p;
      return SPG_TEXT_ERR_BYTE;
    }
  }
}

struct GlobalBytes {
  const u8* text;
  __device__ __forceinline__ unsigned operator()(long p) const { return text[p]; }
};

// error: [0] the lowest refused line (all ones: none), [3] how many lines were refused
__global__ __launch_bounds__(TEXT_BLOCK) void text_parse_kernel(const u8* __restrict__ text, long n, const int64_t* __restrict__ line_start,
                                                                long n_lines, TextCols cols, float* __restrict__ xyz, u8* __restrict__ rgb,
                                                                u8* __restrict__ label, u64* __restrict__ error) {
  const long i = (long)blockIdx.x * TEXT_BLOCK + threadIdx.x;
  if (i >= n_lines) return;
  const long s = line_start[i];
  TextRow row = {0.f, 0.f, 0.f, 0, 0, 0, 0};
  long where = 0;
  int code;
  if (s < 0 || s >= n) code = SPG_TEXT_ERR_BYTE;      // (not an offset into the buffer)
  else code = text_parse_line(GlobalBytes{text}, n, s, cols, &row, &where);
  if (code != 0) {
    row = TextRow{0.f, 0.f, 0.f, 0, 0, 0, 0};
    atomicMin(&error[0], (u64)i);
    atomicAdd(&error[3], (u64)1);
  }
  if (xyz != nullptr) { xyz[3 * i] = row.x; xyz[3 * i + 1] = row.y; xyz[3 * i + 2] = row.z; }
  if (rgb != nullptr) { rgb[3 * i] = row.r; rgb[3 * i + 1] = row.g; rgb[3 * i + 2] = row.b; }
  if (label != nullptr) label[i] = row.label;
}

// the first refused line once more, by one thread: [1] its code, [2] the byte offset
__global__ void text_error_kernel(const u8* __restrict__ text, long n, const int64_t* __restrict__ line_start, long n_lines, TextCols cols,
                                  u64* __restrict__ error) {
  const u64 i = error[0];
  if (i >= (u64)n_lines) return;
  const long s = line_start[i];
  TextRow row;
  long where = s;
  int code = SPG_TEXT_ERR_BYTE;
  if (s >= 0 && s < n) code = text_parse_line(GlobalBytes{text}, n, s, cols, &row, &where);
  error[1] = (u64)code;
  error[2] = (u64)where;
}

struct IndexWs {
  long n_tiles;
  unsigned* counts;
  int64_t* tile_off;
  u64 *tile_nl, *last_nl;      // 1 + the offset of the last '\n' of every tile (0: none), and of the buffer
  void* tmp;
  size_t tmp_bytes;
  IndexWs(Carve& w, long n_bytes) {
    n_tiles = (std::max<long>(n_bytes, 1) + TEXT_INDEX_TILE - 1) / TEXT_INDEX_TILE;
    counts = w.take_n<unsigned>((size_t)n_tiles + 1);
    tile_off = w.take_n<int64_t>((size_t)n_tiles + 1);
    tile_nl = w.take_n<u64>((size_t)n_tiles);
    last_nl = w.take_n<u64>(1);
    size_t reduce_bytes = 0;
    (void)rocprim::reduce(nullptr, reduce_bytes, (u64*)nullptr, (u64*)nullptr, (u64)0, (size_t)n_tiles, rocprim::maximum<u64>(), (hipStream_t)0);
    tmp_bytes = std::max(exclusive_scan_bytes<int64_t>(n_tiles + 1, (unsigned*)nullptr), reduce_bytes);
    tmp = w.take(tmp_bytes);
  }
};

}  // namespace

extern "C" int spg_text_debug_layout(int which) {
  return which == 0 ? TEXT_INDEX_TILE : which == 1 ? TEXT_MAX_LINE : -1;
}

extern "C" size_t spg_text_workspace_bytes(long n_bytes) {
  if (n_bytes < 0 || n_bytes > TEXT_MAX_BYTES) return 0;
  Carve w;
  IndexWs l(w, n_bytes);
  return w.used();
}

extern "C" int spg_text_index(const uint8_t* text, long n_bytes, int final_block, int64_t* head, void* workspace, size_t workspace_bytes,
                              void* stream) {
  SPG_CHECK_ARG(n_bytes >= 0 && n_bytes <= TEXT_MAX_BYTES && head && workspace && (text || n_bytes == 0), "bad argument");
  SPG_CHECK_ARG(((uintptr_t)text & 15) == 0, "text must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  Carve w(workspace, workspace_bytes);
  IndexWs l(w, n_bytes);
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_text_workspace_bytes(n_bytes))");
  SPG_RP(hipMemsetAsync(head, 0, 2 * sizeof(int64_t), st));
  if (n_bytes == 0) return 0;
  SPG_RP(hipMemsetAsync(l.counts + l.n_tiles, 0, sizeof(unsigned), st));
  hipLaunchKernelGGL(text_count_kernel, dim3((unsigned)l.n_tiles), dim3(TEXT_BLOCK), 0, st, text, n_bytes, l.counts, l.tile_nl);
  SPG_LAUNCH_CHECK();
  size_t b = l.tmp_bytes;
  SPG_RP(rocprim::reduce(l.tmp, b, l.tile_nl, l.last_nl, (u64)0, (size_t)l.n_tiles, rocprim::maximum<u64>(), st));
  b = l.tmp_bytes;
  SPG_RP(rocprim::exclusive_scan(l.tmp, b, l.counts, l.tile_off, (int64_t)0, (size_t)(l.n_tiles + 1), rocprim::plus<int64_t>(), st));
  hipLaunchKernelGGL(text_head_kernel, dim3(1), dim3(1), 0, st, text, n_bytes, final_block, (const int64_t*)l.tile_off, l.n_tiles,
                     (const u64*)l.last_nl, head);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_text_lines(const uint8_t* text, long n_bytes, long n_lines, int64_t* line_start, void* workspace, size_t workspace_bytes,
                              void* stream) {
  SPG_CHECK_ARG(n_bytes >= 0 && n_bytes <= TEXT_MAX_BYTES && n_lines >= 0 && n_lines <= n_bytes && workspace && (text || n_bytes == 0) &&
                    (line_start || n_lines == 0),
                "bad argument");
  SPG_CHECK_ARG(((uintptr_t)text & 15) == 0, "text must be 16-byte aligned");
  if (n_lines == 0) return 0;
  Carve w(workspace, workspace_bytes);
  IndexWs l(w, n_bytes);
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_text_workspace_bytes(n_bytes))");
  hipLaunchKernelGGL(text_place_kernel, dim3((unsigned)l.n_tiles), dim3(TEXT_BLOCK), 0, (hipStream_t)stream, text, n_bytes,
                     (const int64_t*)l.tile_off, n_lines, line_start);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_text_parse(const uint8_t* text, long n_bytes, const int64_t* line_start, long n_lines, int n_cols, const int* roles,
                              float* xyz, uint8_t* rgb, uint8_t* label, int64_t* error, void* stream) {
  SPG_CHECK_ARG(n_bytes >= 0 && n_bytes <= TEXT_MAX_BYTES && n_lines >= 0 && n_lines <= n_bytes && error && roles, "bad argument");
  SPG_CHECK_ARG(n_cols >= 1 && n_cols <= SPG_TEXT_MAX_COLS, "1 <= n_cols <= SPG_TEXT_MAX_COLS");
  SPG_CHECK_ARG(((uintptr_t)text & 15) == 0, "text must be 16-byte aligned");
  TextCols cols = {n_cols, 0};
  unsigned seen = 0u;
  for (int c = 0; c < SPG_TEXT_MAX_COLS; ++c) {
    const int r = c < n_cols ? roles[c] : -1;
    SPG_CHECK_ARG(r >= -1 && r <= 6, "a column role outside -1 ... 6");
    if (r >= 0) {
      SPG_CHECK_ARG(!(seen >> r & 1u), "two columns with one role");
      seen |= 1u << r;
    }
    cols.roles |= (u64)(r + 1) << (4 * c);
  }
  SPG_CHECK_ARG((seen & 7u) == 0u || (seen & 7u) == 7u, "xyz needs three columns");
  SPG_CHECK_ARG((seen & 56u) == 0u || (seen & 56u) == 56u, "rgb needs three columns");
  SPG_CHECK_ARG(n_lines == 0 || (text && line_start && ((seen & 7u) == 0u || xyz) && ((seen & 56u) == 0u || rgb) && ((seen & 64u) == 0u || label)),
                "null pointer");
  if (!(seen & 7u)) xyz = nullptr;
  if (!(seen & 56u)) rgb = nullptr;
  if (!(seen & 64u)) label = nullptr;
  hipStream_t st = (hipStream_t)stream;
  SPG_RP(hipMemsetAsync(error, 0xff, sizeof(int64_t), st));
  SPG_RP(hipMemsetAsync(error + 1, 0, 3 * sizeof(int64_t), st));
  if (n_lines == 0) return 0;
  const dim3 grid((unsigned)spg_cdiv(n_lines, TEXT_BLOCK)), blk(TEXT_BLOCK);
  hipLaunchKernelGGL(text_parse_kernel, grid, blk, 0, st, text, n_bytes, line_start, n_lines, cols, xyz, rgb, label, (u64*)error);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(text_error_kernel, dim3(1), dim3(1), 0, st, text, n_bytes, line_start, n_lines, cols, (u64*)error);
  SPG_LAUNCH_CHECK();
  return 0;
}
