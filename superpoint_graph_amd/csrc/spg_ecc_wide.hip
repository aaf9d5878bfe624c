// RNN-ECC at state widths other than 32 (nc = 8, 16, 64, 128): the per-iteration forward / backward step kernels, the per-edge
// filter gradient and -- through the same kernels with agg_in / dcat -- the stand-alone GRUCellEx / LSTMCellEx.
//
// One workgroup (256 threads) owns a BLOCK of NB nodes (spg_wide_block_nodes: 16 at nc <= 16, 8 at 64, 4 at 128) instead of one
// node per wavefront: the cell's matrices no longer fit a lane layout of 64 + 32 gate values, and at nc = 128 they do not fit LDS
// at all (393 KB), so at EVERY width of this unit the weight rows are read through L2 -- a thread owns a gate row (forward) or a
// state column (backward, W^T) and re-uses every weight it has loaded for the nodes of its block, whose vectors sit in LDS.
// What is per node -- the in-edge aggregation, the reverse-CSR gather of the backward, the row normalisation over the G nc
// pre-activations -- is done by one wavefront per node, the block's nodes dealt round-robin to the four waves.  Every sum has a
// fixed order (edges in CSR / reverse-CSR order, k ascending, a fixed shuffle tree): no atomics, bit-reproducible.
// Expressions and their order follow the 32-wide kernels of spg_ecc.hip (reference learning/modules.py:224-251, :280-309):
// the GRU adds its biases BEHIND the row normalisation, the LSTM in front of it.
// No kernel here waits on another workgroup.
// At the end of the file: the one launcher per operation for EVERY width (spg_ecc_step_fwd / _bwd, spg_ecc_edge_wgrad), whose
// case 32 is the launcher of spg_ecc.hip.
#include "spg_ecc.h"

namespace {

__device__ __forceinline__ float wide_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

#define SPG_WIDE_EPS 1e-5f   // nn.InstanceNorm1d(1, eps=1e-5), learning/modules.py:213-214

template <int NC> struct WideBlock { static constexpr int NB = NC <= 16 ? 16 : (NC <= 64 ? 8 : 4); };

// out[n][row] = sum_k W[row][k] v[n][k] (+ bias[row]) for the NB nodes of the block; W [ROWS][NC] in global memory, v [NB][NC]
// in LDS.  A thread owns one row for the nodes n = g, g + NG, ... of its node group; k ascending.
template <int NC, int NB, int ROWS>
__device__ __forceinline__ void wide_rows_dot(const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ sv,
                                              float* __restrict__ out, int ldo) {
  constexpr int NG = ROWS >= SPG_THREADS ? 1 : (SPG_THREADS / ROWS < NB ? SPG_THREADS / ROWS : NB);
  constexpr int NPT = (NB + NG - 1) / NG;
  for (int item = threadIdx.x; item < ROWS * NG; item += SPG_THREADS) {
    const int row = item % ROWS, g = item / ROWS;
    float acc[NPT];
#pragma unroll
    for (int u = 0; u < NPT; ++u) acc[u] = 0.f;
    const f32x4* wr = reinterpret_cast<const f32x4*>(W + (long)row * NC);
#pragma unroll 4
    for (int k4 = 0; k4 < NC / 4; ++k4) {
      const f32x4 w = wr[k4];
#pragma unroll
      for (int u = 0; u < NPT; ++u) {
        const int n = g + u * NG;
        if (n < NB) {
          const f32x4 x = *reinterpret_cast<const f32x4*>(sv + n * NC + 4 * k4);
          acc[u] = fmaf(w[0], x[0], acc[u]); acc[u] = fmaf(w[1], x[1], acc[u]);
          acc[u] = fmaf(w[2], x[2], acc[u]); acc[u] = fmaf(w[3], x[3], acc[u]);
        }
      }
    }
    const float b = bias != nullptr ? bias[row] : 0.f;
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int n = g + u * NG;
      if (n < NB) out[n * ldo + row] = acc[u] + b;
    }
  }
}

// out[n][c] (+)= sum_o W[o][c] g[n][o], o < ROWS ascending: the W^T products of the backward.  A thread owns column c (the lanes
// of a wave read consecutive floats of a weight row) for the nodes of its node group.
template <int NC, int NB, int ROWS, bool ACCUM>
__device__ __forceinline__ void wide_cols_dot(const float* __restrict__ W, const float* __restrict__ sg, int ldg, float* __restrict__ out) {
  constexpr int NG = SPG_THREADS / NC < NB ? SPG_THREADS / NC : NB;
  constexpr int NPT = (NB + NG - 1) / NG;
  for (int item = threadIdx.x; item < NC * NG; item += SPG_THREADS) {
    const int c = item % NC, g = item / NC;
    float acc[NPT];
#pragma unroll
    for (int u = 0; u < NPT; ++u) acc[u] = 0.f;
#pragma unroll 8
    for (int o = 0; o < ROWS; ++o) {
      const float w = W[(long)o * NC + c];
#pragma unroll
      for (int u = 0; u < NPT; ++u) {
        const int n = g + u * NG;
        if (n < NB) acc[u] = fmaf(w, sg[n * ldg + o], acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int n = g + u * NG;
      if (n < NB) {
        if (ACCUM) out[n * NC + c] += acc[u];
        else out[n * NC + c] = acc[u];
      }
    }
  }
}

// per-row (x - mean) / sqrt(var_biased + eps) over the GW values of every node of the block, in place; one wave per node
template <int NB, int GW>
__device__ __forceinline__ void wide_row_norm(float* __restrict__ v, float* __restrict__ rstd_out, int lane, int wave) {
  for (int n = wave; n < NB; n += 4) {
    float* row = v + n * GW;
    float s = 0.f;
    for (int o = lane; o < GW; o += 64) s += row[o];
    const float mean = spg_wave_sum(s) * (1.f / GW);
    float q = 0.f;
    for (int o = lane; o < GW; o += 64) { const float d = row[o] - mean; q += d * d; }
    const float rstd = 1.0f / sqrtf(spg_wave_sum(q) * (1.f / GW) + SPG_WIDE_EPS);
    for (int o = lane; o < GW; o += 64) row[o] = (row[o] - mean) * rstd;
    if (lane == 0) rstd_out[n] = rstd;
  }
}

// through the row normalisation, in place: dg = rstd (du - mean(du) - u mean(du u)); one wave per node
template <int NB, int GW>
__device__ __forceinline__ void wide_row_norm_bwd(float* __restrict__ du, const float* __restrict__ u, const float* __restrict__ rstd,
                                                  int lane, int wave) {
  for (int n = wave; n < NB; n += 4) {
    float* d = du + n * GW;
    const float* uu = u + n * GW;
    float s1 = 0.f, s2 = 0.f;
    for (int o = lane; o < GW; o += 64) { s1 += d[o]; s2 += d[o] * uu[o]; }
    const float m1 = spg_wave_sum(s1) * (1.f / GW), m2 = spg_wave_sum(s2) * (1.f / GW);
    const float r = rstd[n];
    for (int o = lane; o < GW; o += 64) d[o] = r * (d[o] - m1 - uu[o] * m2);
  }
}

// LDS of a block: what the forward of the cell needs ...
template <int NC, int CELL>
struct WideFwdLds {
  static constexpr int G = CELL == SPG_CELL_LSTM ? 4 : 3, GW = G * NC, NB = WideBlock<NC>::NB;
  float a[NB * NC];          // aggregate
  float h[NB * NC];          // state
  float x[NB * NC];          // gated input
  float gin[NB * NC];        // input gate
  float ui[NB * GW];         // (normalised) W_ih x (+ b_ih: LSTM)
  float uh[NB * GW];         // (normalised) W_hh h (+ b_hh: LSTM)
  float rstd_i[NB], rstd_h[NB];
};
// ... and what the backward adds
template <int NC, int CELL>
struct WideBwdLds {
  static constexpr int GW = WideFwdLds<NC, CELL>::GW, NB = WideFwdLds<NC, CELL>::NB;
  float dH[NB * NC];       // total gradient wrt the state produced; later the direct gradient wrt the state consumed
  float dgi[NB * GW];        // dui, then dgi
  float dgh[NB * GW];        // duh, then dgh
  float dx[NB * NC];         // gradient wrt the gated input
  float dpre[NB * NC];       // gradient wrt the input gate's pre-activation
};

// the cell's forward up to the normalised pre-activations, for the NB nodes of the block (f.a and f.h are set; block-wide)
template <int NC, int CELL>
__device__ __forceinline__ void wide_cell_pre(const SpgGruParams& G, WideFwdLds<NC, CELL>& f, int lane, int wave) {
  constexpr int GW = WideFwdLds<NC, CELL>::GW, NB = WideFwdLds<NC, CELL>::NB;
  // input gate: x = sigmoid(W_ig h + b_ig) * a      (learning/modules.py:225-226)
  if (G.ingate) {
    wide_rows_dot<NC, NB, NC>(G.w_ig, G.b_ig, f.h, f.gin, NC);
    __syncthreads();
  }
  for (int t = threadIdx.x; t < NB * NC; t += SPG_THREADS) {
    const float gin = G.ingate ? wide_sigmoid(f.gin[t]) : 1.f;
    f.gin[t] = gin;
    f.x[t] = gin * f.a[t];
  }
  __syncthreads();
  constexpr bool LSTM = CELL == SPG_CELL_LSTM;      // biases in front of the normalisation (:296-297); GRU: behind it (:247-249)
  wide_rows_dot<NC, NB, GW>(G.w_ih, LSTM ? G.b_ih : nullptr, f.x, f.ui, GW);
  wide_rows_dot<NC, NB, GW>(G.w_hh, LSTM ? G.b_hh : nullptr, f.h, f.uh, GW);
  __syncthreads();
  if (G.layernorm) {
    wide_row_norm<NB, GW>(f.ui, f.rstd_i, lane, wave);
    wide_row_norm<NB, GW>(f.uh, f.rstd_h, lane, wave);
    __syncthreads();
  } else if (threadIdx.x < NB) {
    f.rstd_i[threadIdx.x] = 1.f; f.rstd_h[threadIdx.x] = 1.f;
  }
}

// in-edge mean aggregation of node i by one wavefront; result in sa[0 .. NC) (LDS)
template <int NC>
__device__ __forceinline__ void wide_aggregate_node(const SpgGraph& g, const float* __restrict__ W, int matrix, const float* __restrict__ hin,
                                                    long ld, int i, int lane, float* __restrict__ sa) {
  const int e0 = g.rowptr[i], e1 = g.rowptr[i + 1];
  const float s = g.invdeg[i];
  if (matrix) {
    // (matrix filters exist up to SPG_WIDE_MATRIX_MAX_NC = 64 only: spg_wide_check and the launchers below refuse `matrix` at
    //  128, so the branch that is compiled out here can never be asked for -- it would leave sa unwritten)
    if constexpr (NC <= 64) {      // lane = (k group, output channel c); W_e[in k][out c]
      constexpr int KG = 64 / NC;
      const int c = lane % NC, kg = lane / NC;
      float a = 0.f;
      for (int e = e0; e < e1; ++e) {
        const float* We = W + (long)e * NC * NC;
        const float* xj = hin + (long)g.src[e] * ld;
#pragma unroll 4
        for (int k = kg; k < NC; k += KG) a = fmaf(xj[k], We[k * NC + c], a);
      }
#pragma unroll
      for (int off = NC; off < 64; off <<= 1) a += __shfl_xor(a, off, 64);
      if (lane < NC) sa[lane] = a * s;
    }
  } else {
    for (int c = lane; c < NC; c += 64) {
      float a = 0.f;
      for (int e = e0; e < e1; ++e) a = fmaf(hin[(long)g.src[e] * ld + c], W[(long)e * NC + c], a);
      sa[c] = a * s;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// forward step
// ---------------------------------------------------------------------------------------------
template <int NC, int CELL>
__global__ __launch_bounds__(SPG_THREADS) void spg_ecc_wide_step_fwd_kernel(const SpgEccStepFwd p) {
  typedef WideFwdLds<NC, CELL> F;
  constexpr int NB = F::NB;
  __shared__ __attribute__((aligned(16))) F f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = blockIdx.x * NB, N = p.g.N;
  for (int n = wave; n < NB; n += 4) {
    const int i = i0 + n;
    float* sa = f.a + n * NC;
    if (i < N) {
      if (p.agg_in != nullptr) {
        for (int c = lane; c < NC; c += 64) sa[c] = p.agg_in[(long)i * p.ldagg + c];
      } else {
        wide_aggregate_node<NC>(p.g, p.W, p.matrix, p.hin, p.ld, i, lane, sa);
      }
      for (int c = lane; c < NC; c += 64) f.h[n * NC + c] = p.hin[(long)i * p.ld + c];
    } else {
      for (int c = lane; c < NC; c += 64) { sa[c] = 0.f; f.h[n * NC + c] = 0.f; }
    }
  }
  __syncthreads();
  if (p.agg_save != nullptr)
    for (int t = threadIdx.x; t < NB * NC; t += SPG_THREADS) {
      const int n = t / NC, c = t % NC;
      if (i0 + n < N) p.agg_save[(long)(i0 + n) * p.ldagg + c] = f.a[t];
    }
  wide_cell_pre<NC, CELL>(p.gru, f, lane, wave);
  const SpgGruParams& G = p.gru;
  for (int t = threadIdx.x; t < NB * NC; t += SPG_THREADS) {
    const int n = t / NC, c = t % NC, i = i0 + n;
    if (i >= N) continue;
    const float* ui = f.ui + n * F::GW;
    const float* uh = f.uh + n * F::GW;
    if constexpr (CELL == SPG_CELL_GRU) {
      const float r = wide_sigmoid(((ui[c] + G.b_ih[c]) + uh[c]) + G.b_hh[c]);
      const float z = wide_sigmoid(((ui[NC + c] + G.b_ih[NC + c]) + uh[NC + c]) + G.b_hh[NC + c]);
      const float nn = tanhf((ui[2 * NC + c] + G.b_ih[2 * NC + c]) + r * (uh[2 * NC + c] + G.b_hh[2 * NC + c]));
      p.hout[(long)i * p.ld + c] = nn + z * (f.h[t] - nn);      // hy = newgate + inputgate * (hidden - newgate)
    } else {
      const float ig = wide_sigmoid(ui[c] + uh[c]), fg = wide_sigmoid(ui[NC + c] + uh[NC + c]);
      const float gg = tanhf(ui[2 * NC + c] + uh[2 * NC + c]), og = wide_sigmoid(ui[3 * NC + c] + uh[3 * NC + c]);
      const float cp = p.cin != nullptr ? p.cin[(long)i * p.ld + c] : 0.f;
      const float cy = fg * cp + ig * gg;                       // :306
      p.cout[(long)i * p.ld + c] = cy;
      p.hout[(long)i * p.ld + c] = og * tanhf(cy);              // :307
    }
  }
}

// ---------------------------------------------------------------------------------------------
// backward step (the fields of SpgEccStepBwd as in spg_ecc.h, with nc for 32: dhdir / dcdir / gx are [N, nc], ld96 is the leading
// dimension of the G nc wide gate gradients, ld32 that of the nc wide dpre / xg)
// ---------------------------------------------------------------------------------------------
// MATRIX: the launch may gather through matrix filters (p.matrix with a next iteration).  Its nc^2 / 64 partial sums per lane cost
// registers (173 VGPRs at 64), so vector-filter and stand-alone-cell launches run the instantiation without that branch.
template <int NC, int CELL, bool MATRIX>
__global__ __launch_bounds__(SPG_THREADS) void spg_ecc_wide_step_bwd_kernel(const SpgEccStepBwd p) {
  typedef WideFwdLds<NC, CELL> F;
  typedef WideBwdLds<NC, CELL> B;
  constexpr int NB = F::NB, GW = F::GW;
  __shared__ __attribute__((aligned(16))) F f;
  __shared__ __attribute__((aligned(16))) B b;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = blockIdx.x * NB, N = p.g.N;
  // ---- phase 1: total gradient wrt the state produced by this iteration: dcat + dhdir + sum_{out-edges} W_e . Gnext[dst] ----
  for (int n = wave; n < NB; n += 4) {
    const int j = j0 + n;
    float* sd = b.dH + n * NC;
    if (j >= N) {
      for (int c = lane; c < NC; c += 64) sd[c] = 0.f;
      continue;
    }
    if (MATRIX && p.Gnext != nullptr && p.matrix) {
      // (MATRIX is instantiated up to SPG_WIDE_MATRIX_MAX_NC = 64 only: launch_bwd refuses `matrix` at 128)
      if constexpr (MATRIX && NC <= 64) {      // lane = (k group, c): partial sums over the out-edges first, ONE reduction over c at the end
        constexpr int KG = 64 / NC, NQ = NC / KG;
        const int c = lane % NC, kg = lane / NC;
        float acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
        const int t0 = p.g.rev_rowptr[j], t1 = p.g.rev_rowptr[j + 1];
        for (int t = t0; t < t1; ++t) {
          const int e = p.g.rev_eid[t];
          const float gc = p.Gnext[(long)p.g.dst[e] * p.ldg + c];
          const float* We = p.W + (long)e * NC * NC;
#pragma unroll
          for (int q = 0; q < NQ; ++q) acc[q] = fmaf(We[(kg + KG * q) * NC + c], gc, acc[q]);
        }
#pragma unroll
        for (int off = 1; off < NC; off <<= 1) {
#pragma unroll
          for (int q = 0; q < NQ; ++q) acc[q] += __shfl_xor(acc[q], off, 64);
        }
        if (c == 0) {
#pragma unroll
          for (int q = 0; q < NQ; ++q) sd[kg + KG * q] = acc[q];
        }
      }
    } else {
      for (int c = lane; c < NC; c += 64) {
        float s = 0.f;
        if (p.Gnext != nullptr) {
          const int t0 = p.g.rev_rowptr[j], t1 = p.g.rev_rowptr[j + 1];
          for (int t = t0; t < t1; ++t) {
            const int e = p.g.rev_eid[t];
            s = fmaf(p.W[(long)e * NC + c], p.Gnext[(long)p.g.dst[e] * p.ldg + c], s);
          }
        }
        sd[c] = s;
      }
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < NB * NC; t += SPG_THREADS) {
    const int n = t / NC, c = t % NC, j = j0 + n;
    if (j >= N) continue;
    float dH = 0.f;
    if (p.dcat != nullptr) dH += p.dcat[(long)j * p.ldc + c];
    if (p.use_dhdir) dH += p.dhdir[(long)j * NC + c];
    dH += b.dH[t];
    if (p.final_only) p.gx[(long)j * NC + c] = dH;
    else b.dH[t] = dH;
  }
  if (p.final_only) return;
  // ---- phase 2: recompute the cell's forward of this iteration, then its backward ----
  for (int t = threadIdx.x; t < NB * NC; t += SPG_THREADS) {
    const int n = t / NC, c = t % NC, j = j0 + n;
    f.a[t] = j < N ? p.agg[(long)j * p.ldagg + c] : 0.f;
    f.h[t] = j < N ? p.hin[(long)j * p.ld + c] : 0.f;
  }
  __syncthreads();
  const SpgGruParams& G = p.gru;
  wide_cell_pre<NC, CELL>(G, f, lane, wave);
  __syncthreads();
  // gates and the gradients wrt the normalised pre-activations
  for (int t = threadIdx.x; t < NB * NC; t += SPG_THREADS) {
    const int n = t / NC, c = t % NC, j = j0 + n;
    const bool active = j < N;
    const float* ui = f.ui + n * GW;
    const float* uh = f.uh + n * GW;
    float* dui = b.dgi + n * GW;
    float* duh = b.dgh + n * GW;
    const float dH = b.dH[t];
    if constexpr (CELL == SPG_CELL_GRU) {
      const float bhn = G.b_hh[2 * NC + c];
      const float r = wide_sigmoid(((ui[c] + G.b_ih[c]) + uh[c]) + G.b_hh[c]);
      const float z = wide_sigmoid(((ui[NC + c] + G.b_ih[NC + c]) + uh[NC + c]) + G.b_hh[NC + c]);
      const float nn = tanhf((ui[2 * NC + c] + G.b_ih[2 * NC + c]) + r * (uh[2 * NC + c] + bhn));
      const float dn_pre = dH * (1.f - z) * (1.f - nn * nn);
      const float dz_pre = dH * (f.h[t] - nn) * z * (1.f - z);
      const float dr_pre = dn_pre * (uh[2 * NC + c] + bhn) * r * (1.f - r);
      b.dH[t] = dH * z;                      // direct path to the state consumed
      dui[c] = dr_pre; dui[NC + c] = dz_pre; dui[2 * NC + c] = dn_pre;
      duh[c] = dr_pre; duh[NC + c] = dz_pre; duh[2 * NC + c] = dn_pre * r;
      if (active) {      // the biases sit behind the normalisation: their gradients are the column sums of dui / duh
        float* o1 = p.dui + (long)j * p.ld96;
        float* o2 = p.duh + (long)j * p.ld96;
        o1[c] = dr_pre; o1[NC + c] = dz_pre; o1[2 * NC + c] = dn_pre;
        o2[c] = dr_pre; o2[NC + c] = dz_pre; o2[2 * NC + c] = dn_pre * r;
      }
    } else {
      const float ig = wide_sigmoid(ui[c] + uh[c]), fg = wide_sigmoid(ui[NC + c] + uh[NC + c]);
      const float gg = tanhf(ui[2 * NC + c] + uh[2 * NC + c]), og = wide_sigmoid(ui[3 * NC + c] + uh[3 * NC + c]);
      const float cp = (active && p.cin != nullptr) ? p.cin[(long)j * p.ld + c] : 0.f;
      const float tc = tanhf(fg * cp + ig * gg);
      float dC = dH * og * (1.f - tc * tc);
      if (p.use_dcdir && active) dC += p.dcdir[(long)j * NC + c];
      const float do_pre = dH * tc * og * (1.f - og);
      const float di_pre = dC * gg * ig * (1.f - ig);
      const float df_pre = dC * cp * fg * (1.f - fg);
      const float dg_pre = dC * ig * (1.f - gg * gg);
      if (active) p.dcdir[(long)j * NC + c] = dC * fg;
      b.dH[t] = 0.f;
      dui[c] = di_pre; dui[NC + c] = df_pre; dui[2 * NC + c] = dg_pre; dui[3 * NC + c] = do_pre;
      duh[c] = di_pre; duh[NC + c] = df_pre; duh[2 * NC + c] = dg_pre; duh[3 * NC + c] = do_pre;
    }
  }
  __syncthreads();
  if (G.layernorm) {
    wide_row_norm_bwd<NB, GW>(b.dgi, f.ui, f.rstd_i, lane, wave);
    wide_row_norm_bwd<NB, GW>(b.dgh, f.uh, f.rstd_h, lane, wave);
    __syncthreads();
  }
  for (int t = threadIdx.x; t < NB * GW; t += SPG_THREADS) {
    const int n = t / GW, o = t % GW, j = j0 + n;
    if (j < N) {
      p.dgi[(long)j * p.ld96 + o] = b.dgi[t];
      p.dgh[(long)j * p.ld96 + o] = b.dgh[t];
    }
  }
  // dx[c] = sum_o W_ih[o][c] dgi[o];  dh[c] += sum_o W_hh[o][c] dgh[o]
  wide_cols_dot<NC, NB, GW, false>(G.w_ih, b.dgi, GW, b.dx);
  wide_cols_dot<NC, NB, GW, true>(G.w_hh, b.dgh, GW, b.dH);
  __syncthreads();
  for (int t = threadIdx.x; t < NB * NC; t += SPG_THREADS) {
    const int n = t / NC, c = t % NC, j = j0 + n;
    const float dx = b.dx[t], gin = f.gin[t];
    float da = dx, dpre = 0.f;
    if (G.ingate) {
      da = dx * gin;
      dpre = dx * f.a[t] * gin * (1.f - gin);
    }
    b.dpre[t] = dpre;
    if (j < N) {
      p.dpre[(long)j * p.ld32 + c] = dpre;
      p.xg[(long)j * p.ld32 + c] = f.x[t];
      p.Gcur[(long)j * p.ldg + c] = p.g.invdeg != nullptr ? da * p.g.invdeg[j] : da;
    }
  }
  __syncthreads();
  if (G.ingate) {
    wide_cols_dot<NC, NB, NC, true>(G.w_ig, b.dpre, NC, b.dH);
    __syncthreads();
  }
  for (int t = threadIdx.x; t < NB * NC; t += SPG_THREADS) {
    const int n = t / NC, c = t % NC, j = j0 + n;
    if (j < N) p.dhdir[(long)j * NC + c] = b.dH[t];
  }
}

// ---------------------------------------------------------------------------------------------
// per-edge filter gradient, summed over the R iterations in registers (written once): one wavefront per edge
// ---------------------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(SPG_THREADS) void spg_ecc_wide_edge_wgrad_kernel(const SpgEdgeWgrad p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x * 4 + wave;
  if (e >= p.g.E) return;
  const float* hs = p.states + (long)p.g.src[e] * p.lds;
  const float* gd = p.G + (long)p.g.dst[e] * p.ldg;
  if (p.matrix) {
    // (compiled out at 128: launch_edge_wgrad refuses `matrix` there -- dW would stay untouched)
    if constexpr (NC <= 64) {      // dW_e[k][c] = sum_r h^r_src[k] g^r_dst[c]; lane = (k group, c)
      constexpr int KG = 64 / NC, NQ = NC / KG;
      const int c = lane % NC, kg = lane / NC;
      float acc[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
      for (int r = 0; r < p.R; ++r) {
        const float gc = gd[r * NC + c];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = fmaf(hs[r * NC + kg + KG * q], gc, acc[q]);
      }
      float* o = p.dW + (long)e * NC * NC;
#pragma unroll
      for (int q = 0; q < NQ; ++q) o[(kg + KG * q) * NC + c] = acc[q];
    }
  } else {
    for (int c = lane; c < NC; c += 64) {
      float a = 0.f;
      for (int r = 0; r < p.R; ++r) a = fmaf(hs[r * NC + c], gd[r * NC + c], a);
      p.dW[(long)e * NC + c] = a;
    }
  }
}

template <int NC>
int launch_fwd(const SpgEccStepFwd& p, hipStream_t stream) {
  SPG_CHECK_ARG(p.do_gru, "the wide forward step always runs the cell");
  SPG_CHECK_ARG(!(p.matrix && NC > SPG_WIDE_MATRIX_MAX_NC) || p.agg_in != nullptr, "matrix filters at this width");
  const dim3 grid(spg_cdiv(p.g.N, WideBlock<NC>::NB));
  if (p.cell == SPG_CELL_LSTM) hipLaunchKernelGGL((spg_ecc_wide_step_fwd_kernel<NC, SPG_CELL_LSTM>), grid, dim3(SPG_THREADS), 0, stream, p);
  else hipLaunchKernelGGL((spg_ecc_wide_step_fwd_kernel<NC, SPG_CELL_GRU>), grid, dim3(SPG_THREADS), 0, stream, p);
  SPG_LAUNCH_CHECK();
  return 0;
}

template <int NC, bool MATRIX>
int launch_bwd_m(const SpgEccStepBwd& p, hipStream_t stream) {
  const dim3 grid(spg_cdiv(p.g.N, WideBlock<NC>::NB));
  if (p.cell == SPG_CELL_LSTM) hipLaunchKernelGGL((spg_ecc_wide_step_bwd_kernel<NC, SPG_CELL_LSTM, MATRIX>), grid, dim3(SPG_THREADS), 0, stream, p);
  else hipLaunchKernelGGL((spg_ecc_wide_step_bwd_kernel<NC, SPG_CELL_GRU, MATRIX>), grid, dim3(SPG_THREADS), 0, stream, p);
  SPG_LAUNCH_CHECK();
  return 0;
}

template <int NC>
int launch_bwd(const SpgEccStepBwd& p, hipStream_t stream) {
  SPG_CHECK_ARG(!(p.matrix && NC > SPG_WIDE_MATRIX_MAX_NC) || p.Gnext == nullptr, "matrix filters at this width");
  if constexpr (NC <= SPG_WIDE_MATRIX_MAX_NC) {
    if (p.matrix && p.Gnext != nullptr) return launch_bwd_m<NC, true>(p, stream);
  }
  return launch_bwd_m<NC, false>(p, stream);
}

template <int NC>
int launch_edge_wgrad(const SpgEdgeWgrad& p, hipStream_t stream) {      // (its own launch, in stream order; E > 0)
  SPG_CHECK_ARG(!(p.matrix && NC > SPG_WIDE_MATRIX_MAX_NC), "matrix filters at this width");
  hipLaunchKernelGGL(spg_ecc_wide_edge_wgrad_kernel<NC>, dim3(spg_cdiv(p.g.E, 4)), dim3(SPG_THREADS), 0, stream, p);
  SPG_LAUNCH_CHECK();
  return 0;
}

}  // namespace

int spg_wide_check(int nc, int matrix, const char* what) {
  if (nc != 8 && nc != 16 && nc != 32 && nc != 64 && nc != 128) {
    spg_set_error("%s: state width %d is not supported: the HIP RNN-ECC kernels serve widths 8, 16, 32, 64 and 128", what, nc);
    return -2;
  }
  if (matrix && nc > SPG_WIDE_MATRIX_MAX_NC) {
    spg_set_error("%s: matrix filters at state width %d (%d KB of filter per edge) are not supported: matrix filters are limited to "
                  "widths 8, 16, 32 and 64 (use vector filters at 128)", what, nc, nc * nc * 4 / 1024);
    return -2;
  }
  return 0;
}

int spg_wide_block_nodes(int nc) {
  switch (nc) {
    case 8: return WideBlock<8>::NB;
    case 16: return WideBlock<16>::NB;
    case 32: return 4;      // the 32-wide kernels of spg_ecc.hip: one node per wavefront
    case 64: return WideBlock<64>::NB;
    case 128: return WideBlock<128>::NB;
    default: return 4;      // (as before; spg_wide_check is what refuses a width)
  }
}

// ---- one launcher per operation: 32 forwards to the launchers of spg_ecc.hip ----
int spg_ecc_step_fwd(const SpgEccStepFwd& p, int nc, hipStream_t stream) {
  switch (nc) {
    case 8: return launch_fwd<8>(p, stream);
    case 16: return launch_fwd<16>(p, stream);
    case 32: return spg_launch_ecc_step_fwd(p, stream);
    case 64: return launch_fwd<64>(p, stream);
    case 128: return launch_fwd<128>(p, stream);
    default: SPG_CHECK_ARG(false, "forward step: nc must be 8, 16, 32, 64 or 128");
  }
  return 0;
}

int spg_ecc_step_bwd(const SpgEccStepBwd& p, int nc, hipStream_t stream) {
  switch (nc) {
    case 8: return launch_bwd<8>(p, stream);
    case 16: return launch_bwd<16>(p, stream);
    case 32: return spg_launch_ecc_step_bwd(p, stream);
    case 64: return launch_bwd<64>(p, stream);
    case 128: return launch_bwd<128>(p, stream);
    default: SPG_CHECK_ARG(false, "backward step: nc must be 8, 16, 32, 64 or 128");
  }
  return 0;
}

int spg_ecc_edge_wgrad(const SpgGraph& g, int matrix, int nc, const float* states, long lds, const float* G, long ldg, int R,
                       float* dW, hipStream_t stream) {
  if (g.E == 0) return 0;
  SpgEdgeWgrad p;
  p.g = g; p.matrix = matrix; p.states = states; p.lds = lds; p.G = G; p.ldg = ldg; p.R = R; p.dW = dW;
  switch (nc) {
    case 8: return launch_edge_wgrad<8>(p, stream);
    case 16: return launch_edge_wgrad<16>(p, stream);
    case 32: return spg_launch_ecc_edge_wgrad(g, matrix, states, lds, G, ldg, R, dW, stream);      // may join an open grouped launch
    case 64: return launch_edge_wgrad<64>(p, stream);
    case 128: return launch_edge_wgrad<128>(p, stream);
    default: SPG_CHECK_ARG(false, "edge gradient: nc must be 8, 16, 32, 64 or 128");
  }
  return 0;
}
