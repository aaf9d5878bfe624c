// The ground-plane elevation of the learned partition on the device: the reference's supervized_partition/graph_processing.py:181-186
// (and learning/s3dis_dataset.py:130-133) fits sklearn's RANSACRegressor(random_state=0) to the points less than 0.5 above the lowest
// one and takes elevation = z - plane(x, y).  Restated here (tests/plane_restatement.py is the same text in
// numpy).  Two entry points, with the one host read the sizes need (the number of low points) between them:
//
// spg_plane_low   finite check and min z (the two-phase pass of spg_part.h), the flags (z - min z) < low_height in float32, and a
//                 stable compaction of the indices (rocprim::select keeps the order) -> low_index, n_low.
// spg_plane_fit   threshold  two radix sorts of order-preserving float bits and the middle element(s): median(|y - median(y)|) in
//                            float32 with numpy's even rule (a + b) / 2 -- bit for bit.
//                 planes     one lane per trial: the least-squares plane through its three points (centred second moments, 2 x 2;
//                            minimum norm below the cut-off cond = max(rows, 2) * eps_float32 that LinearRegression hands to lstsq
//                            for float32 input), float64, kept as (a, b, centroid).
//                 trials     points x trials.  A workgroup reads its PL_BLOCK * PL_PER_LANE low points ONCE into registers and
//                            runs every trial over them: the plane parameters come from LDS (one broadcast read per trial), the
//                            inlier count goes through ballot / popcount, the three float64 sums of R^2 (r^2, q, q^2 with q = y -
//                            median: shifted, so that the total sum of squares does not cancel) through wave_sum and the four
//                            waves in order (the order of spg_part.h) into partials [blocks][T].
//                 replay     ONE wave: adds the partials block by block (a fixed order), forms R^2 as r2_score does and replays
//                            sklearn's acceptance loop (count < best: skip; equal count and lower score: skip; else accept and
//                            shrink max_trials by _dynamic_max_trials).  No host loop.
//                 final fit  the eight sums of the best trial's inliers by the same two phases; the inlier predicate is the very
//                            function of the trial pass (plane_residual).  Then elevation = z - ((a x + b y) + c) in float64,
//                            rounded once.
// No contraction anywhere (the planes and residuals are the numbers of the restatement, operation by operation), no floating-point
// atomics, no inter-workgroup waiting: two runs give the same bits.
// Error word: bit 0 a coordinate is NaN / infinite, bit 1 no consensus set, bit 2 a subset index outside [0, n_low).
#include <climits>
#include <cmath>
#include <cstring>

#include "../../include/spg_hip.h"
#include "spg_part.h"

namespace {

constexpr int PL_BLOCK = PART_BLOCK;
constexpr int PL_WAVES = PART_WAVES;
constexpr int PL_PER_LANE = 4;
constexpr int PL_POINTS = PL_BLOCK * PL_PER_LANE;     // low points per workgroup of the trial and final passes
constexpr int PL_TILE = 128;                          // trials whose planes and wave sums are in LDS at once
constexpr int PL_MAX_TRIALS = 1024;
constexpr double PL_EPS32 = 1.1920928955078125e-07;   // np.finfo(np.float32).eps
constexpr double PL_EPS64 = 2.220446049250313e-16;    // sklearn's _EPSILON = np.spacing(1)

// ---- low points --------------------------------------------------------------------------------------------------------
// the pass (spg_part.h) of min z and the finite check
struct ZMinPass {
  typedef float T;
  static constexpr int K = 1;
  static constexpr int op(int) { return PART_MIN; }
  float* zmin;
  __device__ void point(const float* __restrict__ xyz, long i, float (&v)[1], int& bad) const {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    bad |= !(finite_f32(x) && finite_f32(y) && finite_f32(z));
    v[0] = fminf(v[0], z);
  }
  __device__ void write(const float (&v)[1], long) const { zmin[0] = v[0]; }
};

__global__ __launch_bounds__(PL_BLOCK) void low_flags_kernel(const float* __restrict__ xyz, long n, const float* __restrict__ zmin,
                                                             float low_height, int32_t* __restrict__ iota, uint8_t* __restrict__ flags) {
  const long i = (long)blockIdx.x * PL_BLOCK + threadIdx.x;
  if (i >= n) return;
  iota[i] = (int32_t)i;
  flags[i] = (xyz[3 * i + 2] - zmin[0]) < low_height;
}

// ---- threshold ---------------------------------------------------------------------------------------------------------
// keys of y = z[low] (med == null) or of |y - *med| in float32
__global__ __launch_bounds__(PL_BLOCK) void keys_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ low_index, long n_low,
                                                        const float* __restrict__ med, unsigned* __restrict__ keys) {
  const long i = (long)blockIdx.x * PL_BLOCK + threadIdx.x;
  if (i >= n_low) return;
  const float y = xyz[3 * (long)low_index[i] + 2];
  keys[i] = ordered_bits(med ? fabsf(y - med[0]) : y);
}

// np.median of the sorted keys: the middle one, or (a + b) / 2 in float32
__global__ void median_kernel(const unsigned* __restrict__ sorted, long n, float* __restrict__ out) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float hi = from_ordered(sorted[n / 2]);
  if (n & 1) { out[0] = hi; return; }
  const float s = from_ordered(sorted[n / 2 - 1]) + hi;
  out[0] = s / 2.f;
}

// ---- least squares -----------------------------------------------------------------------------------------------------
// minimum-norm solution of the centred system from its second moments (LinearRegression.fit: lstsq with cond = max(rows, 2) *
// eps_float32; the eigenvalues of the moments are the squared singular values)
__device__ void solve_centred(double Sxx, double Sxy, double Syy, double Sxz, double Syz, double rows, double& a, double& b) {
#pragma clang fp contract(off)
  a = 0.0; b = 0.0;
  const double cond = fmax(rows, 2.0) * PL_EPS32;
  const double tr = Sxx + Syy;
  if (!(tr > 0.0) || cond >= 1.0) return;
  const double det = Sxx * Syy - Sxy * Sxy;
  const double disc = tr * tr - 4.0 * det;
  const double l1 = (tr + sqrt(disc > 0.0 ? disc : 0.0)) / 2.0;
  if (det > (cond * cond) * (l1 * l1)) {
    a = (Sxz * Syy - Syz * Sxy) / det;
    b = (Syz * Sxx - Sxz * Sxy) / det;
    return;
  }
  double vx = Sxy, vy = l1 - Sxx;            // the eigenvector of l1, from the better conditioned row
  if (fabs(l1 - Syy) > fabs(l1 - Sxx)) { vx = l1 - Syy; vy = Sxy; }
  const double vv = vx * vx + vy * vy;
  if (!(vv > 0.0)) return;
  const double s = (vx * Sxz + vy * Syz) / (vv * l1);
  a = vx * s;
  b = vy * s;
}

// plane: a, b, xr, yr, zr -> |z - ((zr + a (x - xr)) + b (y - yr))|: THE inlier predicate's residual (trial and final pass)
__device__ __forceinline__ double plane_residual(const double* pl, double x, double y, double z) {
#pragma clang fp contract(off)
  const double dx = x - pl[2], dy = y - pl[3];
  const double ax = pl[0] * dx, by = pl[1] * dy;
  const double p = (pl[4] + ax) + by;
  return fabs(z - p);
}

// sum over the three points of d[.][p] * d[.][q], products and sums rounded one by one, left to right
__device__ __forceinline__ double dot3(const double (&d)[3][3], int p, int q) {
#pragma clang fp contract(off)
  const double m0 = d[0][p] * d[0][q], m1 = d[1][p] * d[1][q], m2 = d[2][p] * d[2][q];
  return (m0 + m1) + m2;
}

__global__ __launch_bounds__(64) void planes_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ low_index, long n_low,
                                                    const int32_t* __restrict__ subsets, int T, double* __restrict__ planes,
                                                    int32_t* __restrict__ err) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= T) return;
  double P[3][3];
  int bad = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    long s = subsets[3 * t + j];
    if (s < 0 || s >= n_low) { bad = 1; s = 0; }
    const long i = low_index[s];
#pragma unroll
    for (int c = 0; c < 3; ++c) P[j][c] = (double)xyz[3 * i + c];
  }
  if (bad) atomicOr(err, 4);
  double r[3], d[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    r[c] = ((P[0][c] + P[1][c]) + P[2][c]) / 3.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) d[j][c] = P[j][c] - r[c];
  }
  double a, b;
  solve_centred(dot3(d, 0, 0), dot3(d, 0, 1), dot3(d, 1, 1), dot3(d, 0, 2), dot3(d, 1, 2), 3.0, a, b);
  double* o = planes + 5 * (long)t;
  o[0] = a; o[1] = b; o[2] = r[0]; o[3] = r[1]; o[4] = r[2];
}

// ---- trials ------------------------------------------------------------------------------------------------------------
// the workgroup's PL_POINTS low points into registers (lane-consecutive indices); ok: the point exists
__device__ __forceinline__ void load_points(const float* __restrict__ xyz, const int32_t* __restrict__ low_index, long n_low,
                                            double (&x)[PL_PER_LANE], double (&y)[PL_PER_LANE], double (&z)[PL_PER_LANE],
                                            bool (&ok)[PL_PER_LANE]) {
#pragma unroll
  for (int j = 0; j < PL_PER_LANE; ++j) {
    const long i = (long)blockIdx.x * PL_POINTS + j * PL_BLOCK + threadIdx.x;
    ok[j] = i < n_low;
    const long p = ok[j] ? (long)low_index[i] : 0;
    x[j] = ok[j] ? (double)xyz[3 * p] : 0.0;
    y[j] = ok[j] ? (double)xyz[3 * p + 1] : 0.0;
    z[j] = ok[j] ? (double)xyz[3 * p + 2] : 0.0;
  }
}

__global__ __launch_bounds__(PL_BLOCK) void trials_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ low_index, long n_low,
                                                          const double* __restrict__ planes, int T, const float* __restrict__ med,
                                                          const float* __restrict__ threshold, double* __restrict__ psum,
                                                          int32_t* __restrict__ pcnt) {
#pragma clang fp contract(off)
  __shared__ double pl[PL_TILE][5];
  __shared__ double wsum[PL_WAVES][PL_TILE][3];
  __shared__ int wcnt[PL_WAVES][PL_TILE];
  double x[PL_PER_LANE], y[PL_PER_LANE], z[PL_PER_LANE], q[PL_PER_LANE];
  bool ok[PL_PER_LANE];
  load_points(xyz, low_index, n_low, x, y, z, ok);
  const double m = (double)med[0], thr = (double)threshold[0];
#pragma unroll
  for (int j = 0; j < PL_PER_LANE; ++j) q[j] = z[j] - m;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t0 = 0; t0 < T; t0 += PL_TILE) {
    const int nt = min(PL_TILE, T - t0);
    for (int i = threadIdx.x; i < nt * 5; i += PL_BLOCK) (&pl[0][0])[i] = planes[5 * (long)t0 + i];
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      double s_rr = 0.0, s_q = 0.0, s_qq = 0.0;
      int cnt = 0;
#pragma unroll
      for (int j = 0; j < PL_PER_LANE; ++j) {
        const double r = plane_residual(pl[t], x[j], y[j], z[j]);
        const bool in = ok[j] && r <= thr;
        cnt += __popcll(__ballot(in));
        s_rr += in ? r * r : 0.0;
        s_q += in ? q[j] : 0.0;
        s_qq += in ? q[j] * q[j] : 0.0;
      }
      s_rr = wave_sum(s_rr); s_q = wave_sum(s_q); s_qq = wave_sum(s_qq);
      if (lane == 0) {
        wsum[wave][t][0] = s_rr; wsum[wave][t][1] = s_q; wsum[wave][t][2] = s_qq;
        wcnt[wave][t] = cnt;
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nt * 4; i += PL_BLOCK) {        // the four waves in order
      const int t = i >> 2, c = i & 3;
      const long o = (long)blockIdx.x * T + t0 + t;
      if (c < 3) {
        double s = wsum[0][t][c];
#pragma unroll
        for (int w = 1; w < PL_WAVES; ++w) s += wsum[w][t][c];
        psum[3 * o + c] = s;
      } else {
        int s = wcnt[0][t];
#pragma unroll
        for (int w = 1; w < PL_WAVES; ++w) s += wcnt[w][t];
        pcnt[o] = s;
      }
    }
    __syncthreads();
  }
}

// sklearn's _dynamic_max_trials(count, n_low, 3, 0.99)
__device__ double dynamic_max_trials(double count, double n_low) {
#pragma clang fp contract(off)
  const double ratio = count / n_low;
  const double nom = fmax(PL_EPS64, 1.0 - 0.99);
  const double denom = fmax(PL_EPS64, 1.0 - ratio * ratio * ratio);
  if (denom == 1.0) return INFINITY;
  return fabs(ceil(log(nom) / log(denom)));
}

// one wave: partials -> counts and R^2 per trial (lanes over trials, blocks in order), then lane 0 replays the acceptance loop
__global__ __launch_bounds__(64) void replay_kernel(const double* __restrict__ psum, const int32_t* __restrict__ pcnt, int blocks, int T,
                                                    long n_low, int32_t* __restrict__ result, int32_t* __restrict__ err) {
#pragma clang fp contract(off)
  __shared__ double score[PL_MAX_TRIALS];
  __shared__ int count[PL_MAX_TRIALS];
  for (int t = threadIdx.x; t < T; t += 64) {
    double s_rr = 0.0, s_q = 0.0, s_qq = 0.0;
    int cnt = 0;
    for (int b = 0; b < blocks; ++b) {
      const long o = (long)b * T + t;
      s_rr += psum[3 * o]; s_q += psum[3 * o + 1]; s_qq += psum[3 * o + 2];
      cnt += pcnt[o];
    }
    double r2 = NAN;                                  // r2_score: undefined below two samples
    if (cnt >= 2) {
      const double ss_tot = s_qq - s_q * s_q / (double)cnt;
      if (!(ss_tot > 0.0)) r2 = s_rr == 0.0 ? 1.0 : 0.0;
      else r2 = 1.0 - s_rr / ss_tot;
    }
    score[t] = r2;
    count[t] = cnt;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int n_best = 1, best = -1, t = 0;
  double score_best = -INFINITY, max_trials = (double)T;
  while ((double)t < max_trials) {
    const int c = count[t];
    const double s = score[t];
    ++t;
    if (c < n_best) continue;
    if (c == n_best && s < score_best) continue;
    n_best = c; score_best = s; best = t - 1;
    max_trials = fmin(max_trials, dynamic_max_trials((double)n_best, (double)n_low));
  }
  result[0] = t;
  result[1] = best;
  if (best < 0) atomicOr(err, 2);
}

// ---- final fit ---------------------------------------------------------------------------------------------------------
// the inliers of the best trial: the mask, and per workgroup the sums of dx, dy, dz, dx dx, dx dy, dy dy, dx dz, dy dz (d = the point
// minus the centroid of the best triple) and the count
__global__ __launch_bounds__(PL_BLOCK) void final_partial_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ low_index,
                                                                 long n_low, const double* __restrict__ planes,
                                                                 const int32_t* __restrict__ result, const float* __restrict__ threshold,
                                                                 uint8_t* __restrict__ inlier_mask, double* __restrict__ fsum,
                                                                 int32_t* __restrict__ fcnt) {
#pragma clang fp contract(off)
  __shared__ double wsum[PL_WAVES][8];
  __shared__ int wcnt[PL_WAVES];
  double x[PL_PER_LANE], y[PL_PER_LANE], z[PL_PER_LANE];
  bool ok[PL_PER_LANE];
  load_points(xyz, low_index, n_low, x, y, z, ok);
  const int best = result[1];
  const double thr = (double)threshold[0];
  double pl[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (best >= 0) {
#pragma unroll
    for (int c = 0; c < 5; ++c) pl[c] = planes[5 * (long)best + c];
  }
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < PL_PER_LANE; ++j) {
    const double r = plane_residual(pl, x[j], y[j], z[j]);
    const bool in = best >= 0 && ok[j] && r <= thr;
    const long i = (long)blockIdx.x * PL_POINTS + j * PL_BLOCK + threadIdx.x;
    if (ok[j]) inlier_mask[i] = in;
    cnt += __popcll(__ballot(in));
    const double dx = x[j] - pl[2], dy = y[j] - pl[3], dz = z[j] - pl[4];
    s[0] += in ? dx : 0.0; s[1] += in ? dy : 0.0; s[2] += in ? dz : 0.0;
    s[3] += in ? dx * dx : 0.0; s[4] += in ? dx * dy : 0.0; s[5] += in ? dy * dy : 0.0;
    s[6] += in ? dx * dz : 0.0; s[7] += in ? dy * dz : 0.0;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    s[c] = wave_sum(s[c]);
    if (lane == 0) wsum[wave][c] = s[c];
  }
  if (lane == 0) wcnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x < 8) {
    double v = wsum[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < PL_WAVES; ++w) v += wsum[w][threadIdx.x];
    fsum[8 * (long)blockIdx.x + threadIdx.x] = v;
  } else if (threadIdx.x == 8) {
    int v = wcnt[0];
#pragma unroll
    for (int w = 1; w < PL_WAVES; ++w) v += wcnt[w];
    fcnt[blockIdx.x] = v;
  }
}

// one wave: the partials block by block (lane c < 8 takes sum c, lane 8 the count), the solve, coef, intercept
__global__ __launch_bounds__(64) void final_solve_kernel(const double* __restrict__ fsum, const int32_t* __restrict__ fcnt, int blocks,
                                                         const double* __restrict__ planes, const int32_t* __restrict__ result,
                                                         double* __restrict__ coef, double* __restrict__ intercept) {
#pragma clang fp contract(off)
  __shared__ double S[8];
  __shared__ int N;
  if (threadIdx.x < 8) {
    double v = 0.0;
    for (int b = 0; b < blocks; ++b) v += fsum[8 * (long)b + threadIdx.x];
    S[threadIdx.x] = v;
  } else if (threadIdx.x == 8) {
    int v = 0;
    for (int b = 0; b < blocks; ++b) v += fcnt[b];
    N = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int best = result[1];
  if (best < 0 || N < 1) { coef[0] = NAN; coef[1] = NAN; intercept[0] = NAN; return; }
  const double* ref = planes + 5 * (long)best + 2;
  const double n = (double)N;
  double a, b;
  solve_centred(S[3] - S[0] * S[0] / n, S[4] - S[0] * S[1] / n, S[5] - S[1] * S[1] / n, S[6] - S[0] * S[2] / n, S[7] - S[1] * S[2] / n, n, a, b);
  const double xm = ref[0] + S[0] / n, ym = ref[1] + S[1] / n, zm = ref[2] + S[2] / n;
  coef[0] = a; coef[1] = b;
  const double ax = a * xm, by = b * ym;
  intercept[0] = (zm - ax) - by;
}

__global__ __launch_bounds__(PL_BLOCK) void elevation_kernel(const float* __restrict__ xyz, long n, const double* __restrict__ coef,
                                                             const double* __restrict__ intercept, float* __restrict__ elevation) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * PL_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double x = (double)xyz[3 * i], y = (double)xyz[3 * i + 1], z = (double)xyz[3 * i + 2];
  const double ax = coef[0] * x, by = coef[1] * y;
  elevation[i] = (float)(z - ((ax + by) + intercept[0]));
}

// ---- workspaces --------------------------------------------------------------------------------------------------------
struct LowWs {
  float *zpart, *zmin;       // [blocks], [1]
  int32_t* iota;             // [n]
  uint8_t* flags;            // [n]
  void* tmp;
  size_t tmp_bytes;
  int blocks;
  LowWs(Carve& w, long n) {
    blocks = part_reduce_blocks(n);
    zpart = w.take_n<float>((size_t)blocks);
    zmin = w.take_n<float>(1);
    iota = w.take_n<int32_t>((size_t)n);
    flags = w.take_n<uint8_t>((size_t)n);
    tmp_bytes = select_bytes<int32_t, uint8_t>(n);
    tmp = w.take(tmp_bytes);
  }
};

struct FitWs {
  unsigned *keys0, *keys1;   // [n_low]
  void* tmp;
  size_t tmp_bytes;
  float* med;                // [1]
  double* planes;            // [T, 5]
  double* psum;              // [blocks, T, 3]
  int32_t* pcnt;             // [blocks, T]
  double* fsum;              // [blocks, 8]
  int32_t* fcnt;             // [blocks]
  int blocks;
  FitWs(Carve& w, long n_low, int T) {
    blocks = spg_cdiv(std::max<long>(n_low, 1), PL_POINTS);
    keys0 = w.take_n<unsigned>((size_t)n_low);
    keys1 = w.take_n<unsigned>((size_t)n_low);
    tmp_bytes = radix_sort_keys_bytes<unsigned>(n_low, 0, 32);
    tmp = w.take(tmp_bytes);
    med = w.take_n<float>(1);
    planes = w.take_n<double>((size_t)T * 5);
    psum = w.take_n<double>((size_t)blocks * T * 3);
    pcnt = w.take_n<int32_t>((size_t)blocks * T);
    fsum = w.take_n<double>((size_t)blocks * 8);
    fcnt = w.take_n<int32_t>((size_t)blocks);
  }
};

}  // namespace

extern "C" size_t spg_plane_workspace_bytes(long n, long n_low, int trials) {
  Carve w;
  if (n_low < 0) { LowWs l(w, n); } else { FitWs l(w, n_low, trials); }
  return w.used();
}

extern "C" int spg_plane_low(const float* xyz, long n, float low_height, int32_t* low_index, int32_t* n_low, int32_t* error_flag,
                             void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(xyz && low_index && n_low && error_flag && workspace, "bad argument");
  SPG_CHECK_ARG(n >= 1 && n < INT_MAX, "1 <= n < 2^31 - 1");
  Carve w(workspace, workspace_bytes);
  LowWs l(w, n);
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_plane_workspace_bytes(n, -1, 0))");
  hipStream_t st = (hipStream_t)stream;
  SPG_RP(hipMemsetAsync(error_flag, 0, sizeof(int32_t), st));
  if (int rc = part_reduce(ZMinPass{l.zmin}, xyz, n, l.zpart, l.blocks, error_flag, st)) return rc;
  hipLaunchKernelGGL(low_flags_kernel, dim3(spg_cdiv(n, PL_BLOCK)), dim3(PL_BLOCK), 0, st, xyz, n, (const float*)l.zmin, low_height, l.iota,
                     l.flags);
  SPG_LAUNCH_CHECK();
  size_t b = l.tmp_bytes;
  SPG_RP(rocprim::select(l.tmp, b, l.iota, l.flags, low_index, n_low, (size_t)n, st));
  return 0;
}

extern "C" int spg_plane_fit(const float* xyz, long n, const int32_t* low_index, long n_low, const int32_t* subsets, int trials,
                             float* elevation, double* coef, double* intercept, float* threshold, uint8_t* inlier_mask, int32_t* result,
                             int32_t* error_flag, void* workspace, size_t workspace_bytes, void* stream) {
  SPG_CHECK_ARG(xyz && low_index && subsets && elevation && coef && intercept && threshold && inlier_mask && result && error_flag && workspace,
                "bad argument");
  SPG_CHECK_ARG(n >= 1 && n < INT_MAX && n_low >= 3 && n_low <= n, "1 <= n < 2^31 - 1, 3 <= n_low <= n");
  SPG_CHECK_ARG(trials >= 1 && trials <= PL_MAX_TRIALS, "1 <= trials <= 1024");
  Carve w(workspace, workspace_bytes);
  FitWs l(w, n_low, trials);
  SPG_CHECK_ARG(w.ok, "workspace too small (spg_plane_workspace_bytes(n, n_low, trials))");
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(PL_BLOCK), low_grid(spg_cdiv(n_low, PL_BLOCK));
  for (int pass = 0; pass < 2; ++pass) {          // median(y), then median(|y - median(y)|)
    float* out = pass == 0 ? l.med : threshold;
    hipLaunchKernelGGL(keys_kernel, low_grid, blk, 0, st, xyz, low_index, n_low, pass == 0 ? (const float*)nullptr : (const float*)l.med, l.keys0);
    SPG_LAUNCH_CHECK();
    size_t b = l.tmp_bytes;
    SPG_RP(rocprim::radix_sort_keys(l.tmp, b, (const unsigned*)l.keys0, l.keys1, (size_t)n_low, 0, 32, st));
    hipLaunchKernelGGL(median_kernel, dim3(1), dim3(64), 0, st, (const unsigned*)l.keys1, n_low, out);
    SPG_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(planes_kernel, dim3(spg_cdiv(trials, 64)), dim3(64), 0, st, xyz, low_index, n_low, subsets, trials, l.planes, error_flag);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(trials_kernel, dim3(l.blocks), blk, 0, st, xyz, low_index, n_low, (const double*)l.planes, trials, (const float*)l.med,
                     (const float*)threshold, l.psum, l.pcnt);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(replay_kernel, dim3(1), dim3(64), 0, st, (const double*)l.psum, (const int32_t*)l.pcnt, l.blocks, trials, n_low, result,
                     error_flag);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(final_partial_kernel, dim3(l.blocks), blk, 0, st, xyz, low_index, n_low, (const double*)l.planes, (const int32_t*)result,
                     (const float*)threshold, inlier_mask, l.fsum, l.fcnt);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(final_solve_kernel, dim3(1), dim3(64), 0, st, (const double*)l.fsum, (const int32_t*)l.fcnt, l.blocks,
                     (const double*)l.planes, (const int32_t*)result, coef, intercept);
  SPG_LAUNCH_CHECK();
  hipLaunchKernelGGL(elevation_kernel, dim3(spg_cdiv(n, PL_BLOCK)), blk, 0, st, xyz, n, (const double*)coef, (const double*)intercept, elevation);
  SPG_LAUNCH_CHECK();
  return 0;
}
