// GroupNorm / LayerNorm PointNet of the learned partition's local embedder (reference learning/pointnet.py:24-49, 75-118 with
// norm = 'layer' | 'group'): conv -> GroupNorm -> ReLU per 1x1 convolution, max-pool over the points, concatenated global
// features, FC head (GroupNorm + ReLU after every FC but the last).  Group statistics belong to ONE cloud, so a workgroup takes
// its clouds from the input to the embedding without an activation leaving LDS; train and eval are the same function.
//
// Shape
//   A workgroup of NW wavefronts (NW in {4, 2, 1}, the largest whose LDS layout fits) owns runs of GN_RUN = 32 consecutive
//   clouds (run = blockIdx.x, + gridDim.x, ...).  Convolutions: wave w takes clouds w, w + NW, ... of the run, each through the
//   whole stack in a wave-private LDS region (no workgroup barrier), and leaves the pooled row in a shared [32 x (C + nglobal)]
//   matrix.  FC head: the run's rows as ONE <= 32-row tile, the 32-column output tiles dealt to the waves.
//   Products: v_mfma_f32_32x32x2_f32, one 32 x 32 output tile per call, both operands masked element by element (widths such as
//   34 or 139 and 20 points need no padding; LDS strides are odd, so 32 consecutive rows hit 32 banks).
//   Statistics of a (cloud, group) -- or (row, group) in the head: one wavefront, lane i takes elements i, i + 64, ... in the
//   order (point, channel in group), float64 partial sums, xor-butterfly 32, 16, 8, 4, 2, 1 (every lane ends with the same bits);
//   mean first, then the sum of squared deviations from it; rstd = float(1 / sqrt(var + eps)) in float64, rounded once.
//   Backward: per run the head first (recomputed from the saved pooled rows and statistics), then per cloud the convolution
//   stack is recomputed from the cloud and the saved statistics, and back-propagated.  Every wavefront owns one parameter slot
//   [all dW, db, dgamma, dbeta] in HBM and adds its clouds' contributions in program order; one launch sums the slots in slot
//   order in float64.  No atomics anywhere: two runs give the same bits.
#include "../../include/spg_hip.h"
#include "spg_common.h"
#include <float.h>

namespace {

constexpr int GN_RUN = 32;               // clouds of a run = rows of the head's tile
constexpr int GN_MAX_GRID = 256;         // workgroups of the backward (each wave owns a parameter slot: independent of B)
constexpr int GN_LDS_BYTES = 160 * 1024; // LDS of a gfx950 compute unit
constexpr int GN_ERR_UNSUPPORTED = -2;

struct GnLayer {
  const float *W, *b, *gam, *bet;
  int cin, cout, norm;
  int poff;      // parameter slot: dW at poff, db at poff + cout * cin, dgamma / dbeta behind it
  int soff;      // statistics of this layer inside a cloud's record (2 floats per group)
  int yoff, ldy; // LDS: output buffer of this layer (floats, relative to the region it lives in)
};

struct GnArgs {
  GnLayer conv[SPG_MAX_LAYERS], fc[SPG_MAX_LAYERS];
  int nconv, nfc, nfeat, npts, nglob, G, B, D;
  float eps;
  const float *clouds, *glob, *T;
  float* emb;
  float* ws;                       // [B][rec]: statistics, pooled values, arg-max points of every cloud
  int rec, pool_off, arg_off;
  // LDS layout (float offsets).  Per-wave convolution region:
  int convbase, conv_region, x0off, ldx0, actoff, ldact, goff, g2off, ldg, cstat;
  // shared: pooled matrix, its gradient, head buffers (fc[k].yoff is relative to fcbase)
  int pooloff, dpooloff, ldp, fcbase, factoff, fgoff, fg2off, ldf, fstat;
  // backward
  const float* grad_emb;
  float* slots;
  int nparam;
  float *grad_clouds, *grad_T, *grad_glob;
};

struct Team {       // the lanes that share one piece of work: a wavefront (convolutions) or the workgroup (head)
  int lane, wid, nw;
  bool wg;
};

__device__ __forceinline__ void team_sync(const Team& t) {
  if (t.wg) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one 32 x 32 tile of A[M, K] * B[K, N]: A(m, k) = A[m * sam + k * sak], B(k, n) = Bm[k * sbk + n * sbn]; elements outside the
// matrices are zeros (selected, never multiplied: what lies there may be anything).  Lane (r, h) feeds A(m0 + r, k + h) and
// B(k + h, n0 + r); the reduction runs k = 0, 2, 4, ... in order.  Result: acc[q] = C(m0 + spg_acc_row(q, h), n0 + r).
__device__ __forceinline__ f32x16 gn_tile(const float* A, int sam, int sak, int M, const float* Bm, int sbk, int sbn, int N, int K,
                                          int m0, int n0, int lane) {
  const int r = lane & 31, h = lane >> 5;
  const int m = m0 + r, n = n0 + r;
  const bool mv = m < M, nv = n < N;
  const float* ap = A + (long)(mv ? m : 0) * sam;
  const float* bp = Bm + (long)(nv ? n : 0) * sbn;
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  for (int k0 = 0; k0 < K; k0 += 2) {
    const int k = k0 + h;
    const bool kv = k < K;
    const int kk = kv ? k : 0;
    float a = ap[(long)kk * sak], b = bp[(long)kk * sbk];
    a = (mv && kv) ? a : 0.f;
    b = (nv && kv) ? b : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// out[M, cout] = in[M, cin] * W^T + b (raw layer output)
__device__ __forceinline__ void gn_linear(const Team& t, const float* in, int ldin, int M, const GnLayer& L, float* out, int ldo) {
  const int nrt = (M + 31) >> 5, nct = (L.cout + 31) >> 5;
  for (int tile = t.wid; tile < nrt * nct; tile += t.nw) {
    const int rt = tile / nct, ct = tile - rt * nct;
    const f32x16 acc = gn_tile(in, ldin, 1, M, L.W, 1, L.cin, L.cout, L.cin, 32 * rt, 32 * ct, t.lane);
    const int col = 32 * ct + (t.lane & 31), h = t.lane >> 5;
    if (col < L.cout) {
      const float b = L.b != nullptr ? L.b[col] : 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = 32 * rt + spg_acc_row(q, h);
        if (row < M) out[row * ldo + col] = acc[q] + b;
      }
    }
  }
}

// GroupNorm + ReLU of Y [nrb * rpd rows, cout]: one statistic per (row block, group) over rpd rows x cout / G channels.
// Forward: statistics computed and saved, Y becomes the activation.  Backward's recomputation: statistics read back, Y becomes
// xhat (what the gradient needs) and the activation goes to `act`.
template <bool BWD>
__device__ __forceinline__ void gn_norm(const Team& t, float* Y, int ldy, int nrb, int rpd, const GnLayer& L, int G, float eps,
                                        float* ws0, int rec, float* act, int ldact, bool write_act) {
  const int Cg = L.cout / G, n = rpd * Cg;
  for (int d = t.wid; d < nrb * G; d += t.nw) {
    const int rb = d / G, g = d - rb * G;
    float* base = Y + rb * rpd * ldy + g * Cg;
    float* st = ws0 + (long)rb * rec + L.soff + 2 * g;
    float mean, rstd;
    if (BWD) {
      mean = st[0];
      rstd = st[1];
    } else {
      double s = 0.0;
      for (int e = t.lane; e < n; e += 64) s += (double)base[(e / Cg) * ldy + e % Cg];
      const double mu = wave_sum_f64(s) / (double)n;
      double ss = 0.0;
      for (int e = t.lane; e < n; e += 64) {
        const double dv = (double)base[(e / Cg) * ldy + e % Cg] - mu;
        ss += dv * dv;
      }
      const double var = wave_sum_f64(ss) / (double)n;
      mean = (float)mu;
      rstd = (float)(1.0 / sqrt(var + (double)eps));
      if (t.lane == 0) {
        st[0] = mean;
        st[1] = rstd;
      }
    }
    for (int e = t.lane; e < n; e += 64) {
      const int p = e / Cg, cc = e - p * Cg, c = g * Cg + cc;
      const float xh = (base[p * ldy + cc] - mean) * rstd;
      const float a = fmaxf(fmaf(xh, L.gam[c], L.bet[c]), 0.f);
      if (BWD) {
        base[p * ldy + cc] = xh;
        if (write_act) act[(rb * rpd + p) * ldact + c] = a;
      } else {
        base[p * ldy + cc] = a;
      }
    }
  }
}

// act = ReLU(gamma * xhat + beta): the input of the layer above, again (the same expression as gn_norm: the same bits)
__device__ __forceinline__ void gn_reactivate(const Team& t, const float* Y, int ldy, int M, const GnLayer& L, float* act, int ldact) {
  for (int idx = t.wid * 64 + t.lane; idx < M * L.cout; idx += t.nw * 64) {
    const int p = idx / L.cout, c = idx - p * L.cout;
    act[p * ldact + c] = fmaxf(fmaf(Y[p * ldy + c], L.gam[c], L.bet[c]), 0.f);
  }
}

// Gradient through ReLU + GroupNorm: Gb [rows, cout] holds dL/d activation on entry and dL/d (raw layer output) on return;
// Y holds xhat.  The three terms per group: dz = rstd * (dxh - mean(dxh) - xhat * mean(dxh * xhat)), dxh = du * gamma.
// dgamma / dbeta: one lane per channel, rows in order, float64, added to the wave's parameter slot.
__device__ __forceinline__ void gn_norm_bwd(const Team& t, float* slot, float* Gb, int ldg, const float* Y, int ldy, int nrb, int rpd,
                                            const GnLayer& L, int G, const float* ws0, int rec, float* mstat) {
  const int Cg = L.cout / G, n = rpd * Cg;
  for (int d = t.wid; d < nrb * G; d += t.nw) {
    const int rb = d / G, g = d - rb * G;
    float* gb = Gb + rb * rpd * ldg + g * Cg;
    const float* yb = Y + rb * rpd * ldy + g * Cg;
    double s1 = 0.0, s2 = 0.0;
    for (int e = t.lane; e < n; e += 64) {
      const int p = e / Cg, cc = e - p * Cg, c = g * Cg + cc;
      const float xh = yb[p * ldy + cc], gam = L.gam[c];
      const float du = fmaf(xh, gam, L.bet[c]) > 0.f ? gb[p * ldg + cc] : 0.f;
      gb[p * ldg + cc] = du;
      const float dxh = du * gam;
      s1 += (double)dxh;
      s2 += (double)dxh * (double)xh;
    }
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    if (t.lane == 0) {
      mstat[2 * d] = (float)(s1 / (double)n);
      mstat[2 * d + 1] = (float)(s2 / (double)n);
    }
  }
  team_sync(t);
  const int rows = nrb * rpd;
  float* dgam = slot + L.poff + L.cout * L.cin + L.cout;
  for (int c = t.wid * 64 + t.lane; c < L.cout; c += t.nw * 64) {
    double dg = 0.0, db = 0.0;
    for (int row = 0; row < rows; ++row) {
      const float du = Gb[row * ldg + c];
      dg += (double)du * (double)Y[row * ldy + c];
      db += (double)du;
    }
    dgam[c] += (float)dg;
    dgam[L.cout + c] += (float)db;
  }
  team_sync(t);
  for (int d = t.wid; d < nrb * G; d += t.nw) {
    const int rb = d / G, g = d - rb * G;
    float* gb = Gb + rb * rpd * ldg + g * Cg;
    const float* yb = Y + rb * rpd * ldy + g * Cg;
    const float rstd = ws0[(long)rb * rec + L.soff + 2 * g + 1], m1 = mstat[2 * d], m2 = mstat[2 * d + 1];
    for (int e = t.lane; e < n; e += 64) {
      // never contracted: dxh is rounded as in the sums above before m1 is subtracted.  A group of ONE element has dxh == m1 and
      // xh == 0, and its dz (with everything below it) is then exactly 0; fused, it is rstd times the product's rounding error
#pragma clang fp contract(off)
      const int p = e / Cg, cc = e - p * Cg, c = g * Cg + cc;
      const float xh = yb[p * ldy + cc];
      const float dxh = gb[p * ldg + cc] * L.gam[c];
      gb[p * ldg + cc] = rstd * ((dxh - m1) - xh * m2);
    }
  }
  team_sync(t);
}

// Through the linear map: Gb [M, cout] = dL/d (raw output).  db and dW are added to the wave's slot; dL/d input -> din.
__device__ __forceinline__ void gn_linear_bwd(const Team& t, float* slot, const float* Gb, int ldg, int M, const GnLayer& L,
                                              const float* in, int ldin, float* din, int lddin, bool want_din) {
  float* db = slot + L.poff + L.cout * L.cin;
  for (int c = t.wid * 64 + t.lane; c < L.cout; c += t.nw * 64) {
    double s = 0.0;
    for (int row = 0; row < M; ++row) s += (double)Gb[row * ldg + c];
    db[c] += (float)s;
  }
  const int nmt = (L.cout + 31) >> 5, nnt = (L.cin + 31) >> 5;
  const int r = t.lane & 31, h = t.lane >> 5;
  for (int tile = t.wid; tile < nmt * nnt; tile += t.nw) {      // dW = Gb^T * in: reduction over the rows
    const int mt = tile / nnt, nt = tile - mt * nnt;
    const f32x16 acc = gn_tile(Gb, 1, ldg, L.cout, in, ldin, 1, L.cin, M, 32 * mt, 32 * nt, t.lane);
    const int col = 32 * nt + r;
    if (col < L.cin) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = 32 * mt + spg_acc_row(q, h);
        if (m < L.cout) slot[L.poff + m * L.cin + col] += acc[q];
      }
    }
  }
  if (!want_din) return;
  const int nrt = (M + 31) >> 5;
  for (int tile = t.wid; tile < nrt * nnt; tile += t.nw) {      // din = Gb * W: reduction over the output channels
    const int rt = tile / nnt, nt = tile - rt * nnt;
    const f32x16 acc = gn_tile(Gb, ldg, 1, M, L.W, L.cin, 1, L.cin, L.cout, 32 * rt, 32 * nt, t.lane);
    const int col = 32 * nt + r;
    if (col < L.cin) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = 32 * rt + spg_acc_row(q, h);
        if (row < M) din[row * lddin + col] = acc[q];
      }
    }
  }
}

// the convolution stack of one cloud, by one wavefront in its own LDS region
template <bool BWD>
__device__ __forceinline__ void gn_conv_forward(const GnArgs& a, const Team& t, float* region, float* pool, long cloud, int row) {
  const int P = a.npts;
  float* X0 = region + a.x0off;
  const float* cl = a.clouds + cloud * a.nfeat * P;
  float T0 = 1.f, T1 = 0.f, T2 = 0.f, T3 = 1.f;
  if (a.T != nullptr) {
    const float* T = a.T + cloud * 4;
    T0 = T[0] + 1.f; T1 = T[1]; T2 = T[2]; T3 = T[3] + 1.f;
  }
  for (int idx = t.lane; idx < P * a.nfeat; idx += 64) {
    const int c = idx / P, p = idx - c * P;
    float v = cl[idx];
    if (a.T != nullptr && c < 2) {      // learning/pointnet.py:199  [x y] @ T, the expression of spg_fetch (spg_common.h)
      const float x = cl[p], y = cl[P + p];
      v = c == 0 ? fmaf(x, T0, y * T2) : fmaf(x, T1, y * T3);
    }
    X0[p * a.ldx0 + c] = v;
  }
  team_sync(t);
  float* ws0 = a.ws + cloud * a.rec;
  const float* in = X0;
  int ldin = a.ldx0;
  for (int l = 0; l < a.nconv; ++l) {
    const GnLayer& L = a.conv[l];
    float* Y = region + L.yoff;
    gn_linear(t, in, ldin, P, L, Y, L.ldy);
    team_sync(t);
    gn_norm<BWD>(t, Y, L.ldy, 1, P, L, a.G, a.eps, ws0, a.rec, region + a.actoff, a.ldact, l + 1 < a.nconv);      // (the pooled layer's activation: saved by the forward)
    team_sync(t);
    in = BWD ? region + a.actoff : Y;
    ldin = BWD ? a.ldact : L.ldy;
  }
  if (!BWD) {      // max over the points; the first of equal values wins (torch's max_pool1d)
    const int C = a.conv[a.nconv - 1].cout;
    for (int c = t.lane; c < C; c += 64) {
      float best = in[c];
      int arg = 0;
      for (int p = 1; p < P; ++p) {
        const float v = in[p * ldin + c];
        if (v > best) { best = v; arg = p; }
      }
      pool[row * a.ldp + c] = best;
      ws0[a.pool_off + c] = best;
      reinterpret_cast<int*>(ws0)[a.arg_off + c] = arg;
    }
  }
}

__device__ __forceinline__ void gn_conv_backward(const GnArgs& a, const Team& t, float* slot, float* region, const float* dpool,
                                                 long cloud, int row) {
  const int P = a.npts, CL = a.conv[a.nconv - 1].cout;
  const float* ws0 = a.ws + cloud * a.rec;
  const int* arg = reinterpret_cast<const int*>(ws0) + a.arg_off;
  float* Gb = region + a.goff;
  float* G2 = region + a.g2off;
  for (int idx = t.lane; idx < P * CL; idx += 64) {
    const int p = idx / CL, c = idx - p * CL;
    Gb[p * a.ldg + c] = arg[c] == p ? dpool[row * a.ldp + c] : 0.f;
  }
  team_sync(t);
  const bool want_x = a.grad_clouds != nullptr || a.grad_T != nullptr;
  for (int l = a.nconv - 1; l >= 0; --l) {
    const GnLayer& L = a.conv[l];
    gn_norm_bwd(t, slot, Gb, a.ldg, region + L.yoff, L.ldy, 1, P, L, a.G, ws0, a.rec, region + a.cstat);
    const float* in = region + a.x0off;
    int ldin = a.ldx0;
    if (l > 0) {
      const GnLayer& Lp = a.conv[l - 1];
      gn_reactivate(t, region + Lp.yoff, Lp.ldy, P, Lp, region + a.actoff, a.ldact);
      in = region + a.actoff;
      ldin = a.ldact;
    }
    team_sync(t);
    gn_linear_bwd(t, slot, Gb, a.ldg, P, L, in, ldin, G2, a.ldg, l > 0 || want_x);
    team_sync(t);
    float* sw = Gb; Gb = G2; G2 = sw;
  }
  if (!want_x) return;
  // Gb = gradient wrt the (transformed) cloud [P, nfeat]
  const float* cl = a.clouds + cloud * a.nfeat * P;
  float T0 = 1.f, T1 = 0.f, T2 = 0.f, T3 = 1.f;
  if (a.T != nullptr) {
    const float* T = a.T + cloud * 4;
    T0 = T[0] + 1.f; T1 = T[1]; T2 = T[2]; T3 = T[3] + 1.f;
  }
  if (a.grad_T != nullptr && t.lane < 4) {      // dT[i][j] = sum_p in_i[p] * g_j[p]   (learning/pointnet.py:199)
    const int i = t.lane >> 1, j = t.lane & 1;
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += (double)cl[i * P + p] * (double)Gb[p * a.ldg + j];
    a.grad_T[cloud * 4 + t.lane] = (float)s;
  }
  if (a.grad_clouds != nullptr) {
    float* gc = a.grad_clouds + cloud * a.nfeat * P;
    for (int idx = t.lane; idx < P * a.nfeat; idx += 64) {
      const int c = idx / P, p = idx - c * P;
      float v = Gb[p * a.ldg + c];
      if (a.T != nullptr && c < 2) {
        const float gx = Gb[p * a.ldg], gy = Gb[p * a.ldg + 1];
        v = c == 0 ? fmaf(gx, T0, gy * T1) : fmaf(gx, T2, gy * T3);
      }
      gc[idx] = v;
    }
  }
  team_sync(t);
}

// the head of a run: rows = its nr clouds
template <bool BWD>
__device__ __forceinline__ void gn_fc_forward(const GnArgs& a, const Team& t, float* smem, long cloud0, int nr) {
  const float* in = smem + a.pooloff;
  int ldin = a.ldp;
  float* ws0 = a.ws + cloud0 * a.rec;
  for (int k = 0; k < a.nfc; ++k) {
    const GnLayer& L = a.fc[k];
    const bool last = k + 1 == a.nfc;
    if (BWD && last && !L.norm) break;      // the embedding itself is not needed again
    float* Y = smem + a.fcbase + L.yoff;
    gn_linear(t, in, ldin, nr, L, Y, L.ldy);
    team_sync(t);
    if (L.norm) {
      gn_norm<BWD>(t, Y, L.ldy, nr, 1, L, a.G, a.eps, ws0, a.rec, smem + a.factoff, a.ldf, true);
      team_sync(t);
    }
    if (!BWD && last) {
      for (int idx = t.wid * 64 + t.lane; idx < nr * L.cout; idx += t.nw * 64) {
        const int row = idx / L.cout, c = idx - row * L.cout;
        a.emb[(cloud0 + row) * a.D + c] = Y[row * L.ldy + c];
      }
    }
    in = BWD ? smem + a.factoff : Y;
    ldin = BWD ? a.ldf : L.ldy;
  }
}

__device__ __forceinline__ void gn_stage_globals(const GnArgs& a, const Team& t, float* pool, long cloud0, int nr, bool pooled_too) {
  const int C = a.conv[a.nconv - 1].cout, W = C + a.nglob;
  for (int idx = t.wid * 64 + t.lane; idx < nr * W; idx += t.nw * 64) {
    const int row = idx / W, c = idx - row * W;
    if (c >= C) pool[row * a.ldp + c] = a.glob[(cloud0 + row) * a.nglob + (c - C)];
    else if (pooled_too) pool[row * a.ldp + c] = a.ws[(cloud0 + row) * a.rec + a.pool_off + c];
  }
}

__global__ __launch_bounds__(256) void spg_gn_forward_kernel(const GnArgs a) {
  extern __shared__ float gn_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const Team tw{lane, 0, 1, false}, tg{lane, wave, nw, true};
  float* region = gn_smem + a.convbase + wave * a.conv_region;
  float* pool = gn_smem + a.pooloff;
  const long nruns = ((long)a.B + GN_RUN - 1) / GN_RUN;
  for (long run = blockIdx.x; run < nruns; run += gridDim.x) {
    const long cloud0 = run * GN_RUN;
    const int nr = a.B - cloud0 < GN_RUN ? (int)(a.B - cloud0) : GN_RUN;
    for (int i = wave; i < nr; i += nw) {
      gn_conv_forward<false>(a, tw, region, pool, cloud0 + i, i);
      team_sync(tw);
    }
    gn_stage_globals(a, tg, pool, cloud0, nr, false);
    __syncthreads();
    gn_fc_forward<false>(a, tg, gn_smem, cloud0, nr);
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void spg_gn_backward_kernel(const GnArgs a) {
  extern __shared__ float gn_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const Team tw{lane, 0, 1, false}, tg{lane, wave, nw, true};
  float* region = gn_smem + a.convbase + wave * a.conv_region;
  float* pool = gn_smem + a.pooloff;
  float* dpool = gn_smem + a.dpooloff;
  float* slot = a.slots + ((long)blockIdx.x * nw + wave) * a.nparam;      // this wave's own (zeroed by the host); every address always by the same lane
  const int C = a.conv[a.nconv - 1].cout;
  const long nruns = ((long)a.B + GN_RUN - 1) / GN_RUN;
  for (long run = blockIdx.x; run < nruns; run += gridDim.x) {
    const long cloud0 = run * GN_RUN;
    const int nr = a.B - cloud0 < GN_RUN ? (int)(a.B - cloud0) : GN_RUN;
    // ---- head: recomputed from the saved pooled rows, then back-propagated down to the pooled matrix ----
    gn_stage_globals(a, tg, pool, cloud0, nr, true);
    __syncthreads();
    gn_fc_forward<true>(a, tg, gn_smem, cloud0, nr);
    float* Gb = gn_smem + a.fgoff;
    float* G2 = gn_smem + a.fg2off;
    for (int idx = threadIdx.x; idx < nr * a.D; idx += blockDim.x) {
      const int row = idx / a.D, c = idx - row * a.D;
      Gb[row * a.ldf + c] = a.grad_emb[(cloud0 + row) * a.D + c];
    }
    __syncthreads();
    for (int k = a.nfc - 1; k >= 0; --k) {
      const GnLayer& L = a.fc[k];
      if (L.norm) gn_norm_bwd(tg, slot, Gb, a.ldf, gn_smem + a.fcbase + L.yoff, L.ldy, nr, 1, L, a.G, a.ws + cloud0 * a.rec, a.rec, gn_smem + a.fstat);
      const float* in = pool;
      int ldin = a.ldp;
      if (k > 0) {
        const GnLayer& Lp = a.fc[k - 1];
        gn_reactivate(tg, gn_smem + a.fcbase + Lp.yoff, Lp.ldy, nr, Lp, gn_smem + a.factoff, a.ldf);
        in = gn_smem + a.factoff;
        ldin = a.ldf;
      }
      __syncthreads();
      gn_linear_bwd(tg, slot, Gb, a.ldf, nr, L, in, ldin, k > 0 ? G2 : dpool, k > 0 ? a.ldf : a.ldp, true);
      __syncthreads();
      float* sw = Gb; Gb = G2; G2 = sw;
    }
    if (a.grad_glob != nullptr) {
      for (int idx = threadIdx.x; idx < nr * a.nglob; idx += blockDim.x) {
        const int row = idx / a.nglob, j = idx - row * a.nglob;
        a.grad_glob[(cloud0 + row) * a.nglob + j] = dpool[row * a.ldp + C + j];
      }
    }
    __syncthreads();
    // ---- convolutions: every wave recomputes its clouds (the head's buffers are free: the regions overlay them) ----
    for (int i = wave; i < nr; i += nw) {
      gn_conv_forward<true>(a, tw, region, nullptr, cloud0 + i, i);
      gn_conv_backward(a, tw, slot, region, dpool, cloud0 + i, i);
      team_sync(tw);
    }
    __syncthreads();
  }
}

struct GnReduceJob { float* out; int off, n; };
struct GnReduceArgs { GnReduceJob job[4 * 2 * SPG_MAX_LAYERS]; int njobs, nparam, nslots; const float* slots; };

// parameter gradients: the slots summed in slot order, float64
__global__ void spg_gn_reduce_kernel(const GnReduceArgs r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.nparam) return;
  double s = 0.0;
  for (int k = 0; k < r.nslots; ++k) s += (double)r.slots[(long)k * r.nparam + i];
  for (int j = 0; j < r.njobs; ++j)
    if (i >= r.job[j].off && i < r.job[j].off + r.job[j].n) {
      if (r.job[j].out != nullptr) r.job[j].out[i - r.job[j].off] = (float)s;
      return;
    }
}

#define GN_REFUSE(cond, ...)                \
  do {                                      \
    if (!(cond)) {                          \
      spg_set_error(__VA_ARGS__);           \
      return GN_ERR_UNSUPPORTED;            \
    }                                       \
  } while (0)

struct GnPlan {
  GnArgs a;
  int nw = 0;
  size_t lds_bytes = 0, ws_bytes = 0, bwd_bytes = 0;
  int grid = 0;
};

inline int odd(int v) { return v | 1; }

// layer table, record layout and LDS layout from the configuration; refuses what the kernels do not cover
int gn_plan(const spg_gn_cfg* cfg, int B, bool bwd, GnPlan& pl) {
  SPG_CHECK_ARG(cfg != nullptr && B > 0, "cfg / B");
  const spg_pointnet_cfg& c = cfg->net;
  GnArgs& a = pl.a;
  memset(&a, 0, sizeof(a));
  GN_REFUSE(c.nfeat_stn == 0, "GroupNorm PointNet: an inner STN (nfeat_stn = %d > 0) is not supported; evaluate the STN on its own", c.nfeat_stn);
  GN_REFUSE(c.npts >= 1 && c.npts <= 64, "GroupNorm PointNet: npts = %d is outside the supported range 1 <= npts <= 64", c.npts);
  GN_REFUSE(c.nfeat >= 1 && c.nfeat <= 16, "GroupNorm PointNet: nfeat = %d is outside the supported range 1 <= nfeat <= 16", c.nfeat);
  GN_REFUSE(c.nfeat_global >= 0 && c.nfeat_global <= 64, "GroupNorm PointNet: nfeat_global = %d is outside the supported range 0..64", c.nfeat_global);
  GN_REFUSE(c.n_conv >= 1 && c.n_conv <= SPG_MAX_LAYERS && c.n_fc >= 1 && c.n_fc <= SPG_MAX_LAYERS,
            "GroupNorm PointNet: %d conv / %d fc layers; 1 <= layers <= SPG_MAX_LAYERS = %d per stack", c.n_conv, c.n_fc, SPG_MAX_LAYERS);
  GN_REFUSE(cfg->n_group >= 1, "GroupNorm PointNet: n_group = %d must be >= 1", cfg->n_group);
  a.nconv = c.n_conv; a.nfc = c.n_fc; a.nfeat = c.nfeat; a.npts = c.npts; a.nglob = c.nfeat_global; a.G = cfg->n_group; a.B = B;
  a.eps = cfg->eps; a.D = c.fc[c.n_fc - 1];
  int poff = 0, soff = 0;
  auto fill = [&](GnLayer& L, int cin, int cout, int norm) -> int {
    GN_REFUSE(cout >= 1 && cout <= 128, "GroupNorm PointNet: layer width %d is outside the supported range 1 <= width <= 128", cout);
    GN_REFUSE(!norm || cout % cfg->n_group == 0, "GroupNorm PointNet: n_group = %d does not divide the normalised width %d", cfg->n_group, cout);
    L.cin = cin; L.cout = cout; L.norm = norm; L.poff = poff; L.soff = soff; L.ldy = odd(cout);
    poff += cout * cin + cout + (norm ? 2 * cout : 0);
    soff += norm ? 2 * cfg->n_group : 0;
    return 0;
  };
  for (int l = 0; l < c.n_conv; ++l) SPG_TRY(fill(a.conv[l], l ? c.conv[l - 1] : c.nfeat, c.conv[l], 1));
  const int CL = c.conv[c.n_conv - 1];
  for (int k = 0; k < c.n_fc; ++k) SPG_TRY(fill(a.fc[k], k ? c.fc[k - 1] : CL + c.nfeat_global, c.fc[k], (k + 1 < c.n_fc || c.last_ac) ? 1 : 0));
  a.nparam = poff;
  a.pool_off = soff; a.arg_off = soff + CL; a.rec = soff + 2 * CL;
  pl.ws_bytes = (size_t)B * a.rec * sizeof(float) + 256;

  // ---- LDS: derived from the configuration ----
  const int P = c.npts, G = cfg->n_group;
  int wconv = c.nfeat, wfc = 1, wact = 1;
  for (int l = 0; l < c.n_conv; ++l) { wconv = c.conv[l] > wconv ? c.conv[l] : wconv; if (l + 1 < c.n_conv && c.conv[l] > wact) wact = c.conv[l]; }
  for (int k = 0; k < c.n_fc; ++k) wfc = c.fc[k] > wfc ? c.fc[k] : wfc;
  a.ldx0 = odd(c.nfeat); a.ldact = odd(wact); a.ldg = odd(wconv); a.ldp = odd(CL + c.nfeat_global); a.ldf = odd(wfc);
  int off = 0;
  a.x0off = off; off += P * a.ldx0;
  if (!bwd) {      // two buffers, the layers alternate between them
    int w[2] = {1, 1};
    for (int l = 0; l < c.n_conv; ++l) w[l & 1] = c.conv[l] > w[l & 1] ? c.conv[l] : w[l & 1];
    const int o0 = off, o1 = off + P * odd(w[0]);
    for (int l = 0; l < c.n_conv; ++l) a.conv[l].yoff = (l & 1) ? o1 : o0;
    off = o1 + (c.n_conv > 1 ? P * odd(w[1]) : 0);
  } else {         // every layer keeps its xhat; + activation, two gradient buffers, the groups' two means
    for (int l = 0; l < c.n_conv; ++l) { a.conv[l].yoff = off; off += P * a.conv[l].ldy; }
    a.actoff = off; off += P * a.ldact;
    a.goff = off; off += P * a.ldg;
    a.g2off = off; off += P * a.ldg;
    a.cstat = off; off += 2 * G;
  }
  a.conv_region = off;
  int fcf = 0;     // head buffers, relative to fcbase
  if (!bwd) {
    for (int k = 0; k < c.n_fc; ++k) a.fc[k].yoff = (k & 1) ? GN_RUN * a.ldf : 0;
    fcf = 2 * GN_RUN * a.ldf;
  } else {
    for (int k = 0; k < c.n_fc; ++k) { a.fc[k].yoff = fcf; fcf += GN_RUN * a.fc[k].ldy; }
  }
  int shared = 0;
  if (!bwd) {      // [pooled][head][NW regions]
    a.pooloff = 0; shared = GN_RUN * a.ldp;
    a.fcbase = shared; shared += fcf;
    a.convbase = shared;
  } else {         // [d pooled][ {pooled, head, activation, two gradients, means} | {NW regions} ]
    a.dpooloff = 0; shared = GN_RUN * a.ldp;
    a.convbase = shared;
    a.pooloff = shared; int o = shared + GN_RUN * a.ldp;
    a.fcbase = o; o += fcf;
    a.factoff = o; o += GN_RUN * a.ldf;
    a.fgoff = o; o += GN_RUN * a.ldf;
    a.fg2off = o; o += GN_RUN * a.ldf;
    a.fstat = o; o += 2 * GN_RUN * G;
    fcf = o - shared;      // the head's side of the overlay
  }
  pl.nw = 0;
  for (int nw = 4; nw >= 1; nw >>= 1) {
    const size_t floats = bwd ? (size_t)shared + (size_t)((long)nw * a.conv_region > fcf ? (long)nw * a.conv_region : fcf)
                              : (size_t)shared + (size_t)nw * a.conv_region;
    if (floats * sizeof(float) <= (size_t)GN_LDS_BYTES) { pl.nw = nw; pl.lds_bytes = floats * sizeof(float); break; }
  }
  GN_REFUSE(pl.nw > 0, "GroupNorm PointNet: this configuration needs more than the %d bytes of LDS of a compute unit (%s pass: %d floats per cloud region, %d shared)",
            GN_LDS_BYTES, bwd ? "backward" : "forward", a.conv_region, shared + (bwd ? fcf : 0));
  const long nruns = ((long)B + GN_RUN - 1) / GN_RUN;
  pl.grid = (int)(bwd ? (nruns < GN_MAX_GRID ? nruns : GN_MAX_GRID) : (nruns < 65535 ? nruns : 65535));
  pl.bwd_bytes = (size_t)GN_MAX_GRID * 4 * a.nparam * sizeof(float) + 256;      // a slot per wave of the largest grid: no term in B
  return 0;
}

int gn_bind(GnPlan& pl, const void* const* params) {
  GnArgs& a = pl.a;
  for (int i = 0; i < a.nconv + a.nfc; ++i) {
    GnLayer& L = i < a.nconv ? a.conv[i] : a.fc[i - a.nconv];
    const void* const* g = params + 6 * i;
    L.W = (const float*)g[0]; L.b = (const float*)g[1]; L.gam = (const float*)g[2]; L.bet = (const float*)g[3];
    SPG_CHECK_ARG(L.W != nullptr, "missing layer weight");
    SPG_CHECK_ARG(!L.norm || (L.gam != nullptr && L.bet != nullptr), "missing GroupNorm weight / bias");
  }
  return 0;
}

template <class K>
int gn_allow_lds(K kernel, size_t bytes) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) { spg_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
  return 0;
}

}  // namespace

extern "C" int spg_gn_check(const spg_gn_cfg* cfg) {
  GnPlan f, b;
  SPG_TRY(gn_plan(cfg, 1, false, f));
  return gn_plan(cfg, 1, true, b);
}

extern "C" int spg_gn_debug_waves(const spg_gn_cfg* cfg, int backward) {
  GnPlan pl;
  const int rc = gn_plan(cfg, 1, backward != 0, pl);
  return rc == 0 ? pl.nw : rc;
}

extern "C" size_t spg_gn_workspace_bytes(const spg_gn_cfg* cfg, int B) {
  GnPlan pl;
  return gn_plan(cfg, B, false, pl) == 0 ? pl.ws_bytes : 0;
}

extern "C" size_t spg_gn_bwd_workspace_bytes(const spg_gn_cfg* cfg, int B) {
  GnPlan pl;
  return gn_plan(cfg, B, true, pl) == 0 ? pl.bwd_bytes : 0;
}

extern "C" int spg_gn_forward_ext(const spg_gn_cfg* cfg, int B, const float* clouds, const float* clouds_global, const float* ext_transform,
                                  const void* const* params, float* emb, void* workspace, void* stream) {
  SPG_CHECK_ARG(clouds && params && emb && workspace, "null pointer");
  GnPlan pl;
  SPG_TRY(gn_plan(cfg, B, false, pl));
  SPG_CHECK_ARG(pl.a.nglob == 0 || clouds_global != nullptr, "clouds_global is required");
  SPG_CHECK_ARG(ext_transform == nullptr || pl.a.nfeat >= 2, "an external transform needs the xy rows");
  SPG_TRY(gn_bind(pl, params));
  pl.a.clouds = clouds; pl.a.glob = clouds_global; pl.a.T = ext_transform; pl.a.emb = emb; pl.a.ws = (float*)workspace;
  SPG_TRY(gn_allow_lds(spg_gn_forward_kernel, pl.lds_bytes));
  hipLaunchKernelGGL(spg_gn_forward_kernel, dim3(pl.grid), dim3(64 * pl.nw), pl.lds_bytes, (hipStream_t)stream, pl.a);
  SPG_LAUNCH_CHECK();
  return 0;
}

extern "C" int spg_gn_backward_ext(const spg_gn_cfg* cfg, int B, const float* clouds, const float* clouds_global, const float* ext_transform,
                                   const void* const* params, const float* grad_emb, void* const* grads, float* grad_transform,
                                   float* grad_global, float* grad_clouds, void* workspace, void* bwd_workspace, void* stream) {
  SPG_CHECK_ARG(clouds && params && grad_emb && grads && workspace && bwd_workspace, "null pointer");
  SPG_CHECK_ARG(grad_transform == nullptr || ext_transform != nullptr, "grad_transform needs the external transform");
  GnPlan pl;
  SPG_TRY(gn_plan(cfg, B, true, pl));
  SPG_CHECK_ARG(pl.a.nglob == 0 || clouds_global != nullptr, "clouds_global is required");
  SPG_CHECK_ARG(ext_transform == nullptr || pl.a.nfeat >= 2, "an external transform needs the xy rows");
  SPG_TRY(gn_bind(pl, params));
  GnArgs& a = pl.a;
  a.clouds = clouds; a.glob = clouds_global; a.T = ext_transform; a.ws = (float*)workspace;
  a.grad_emb = grad_emb; a.slots = (float*)bwd_workspace; a.grad_clouds = grad_clouds; a.grad_T = grad_transform;
  a.grad_glob = a.nglob > 0 ? grad_global : nullptr;
  hipStream_t st = (hipStream_t)stream;
  SPG_TRY(gn_allow_lds(spg_gn_backward_kernel, pl.lds_bytes));
  hipError_t me = hipMemsetAsync(a.slots, 0, (size_t)pl.grid * pl.nw * a.nparam * sizeof(float), st);
  if (me != hipSuccess) { spg_set_error("hipMemsetAsync: %s", hipGetErrorString(me)); return (int)me; }
  hipLaunchKernelGGL(spg_gn_backward_kernel, dim3(pl.grid), dim3(64 * pl.nw), pl.lds_bytes, st, a);
  SPG_LAUNCH_CHECK();
  GnReduceArgs r;
  memset(&r, 0, sizeof(r));
  for (int i = 0; i < a.nconv + a.nfc; ++i) {
    const GnLayer& L = i < a.nconv ? a.conv[i] : a.fc[i - a.nconv];
    void* const* g = grads + 6 * i;
    r.job[r.njobs++] = GnReduceJob{(float*)g[0], L.poff, L.cout * L.cin};
    r.job[r.njobs++] = GnReduceJob{(float*)g[1], L.poff + L.cout * L.cin, L.cout};
    if (L.norm) {
      r.job[r.njobs++] = GnReduceJob{(float*)g[2], L.poff + L.cout * L.cin + L.cout, L.cout};
      r.job[r.njobs++] = GnReduceJob{(float*)g[3], L.poff + L.cout * L.cin + 2 * L.cout, L.cout};
    }
  }
  r.nparam = a.nparam; r.nslots = pl.grid * pl.nw; r.slots = a.slots;
  hipLaunchKernelGGL(spg_gn_reduce_kernel, dim3(spg_cdiv(a.nparam, 256)), dim3(256), 0, st, r);
  SPG_LAUNCH_CHECK();
  return 0;
}
