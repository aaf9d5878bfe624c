// One BatchNorm dense layer on the few-row GEMMs (spg_gemm.h): the layer record, its operands, the BatchNorm hand-over between
// producer and consumer, and the forward / backward launch recipes shared by PointNet's FC heads (spg_pointnet.hip) and the
// filter-generating network (spg_eccnet.hip).  Host code only; the protocol is stated once in DESIGN 4.5a.
#pragma once
#include "spg_gemm.h"

struct SpgDenseLayer {
  int cin = 0, cout = 0;
  bool bn = false, relu = false;     // BatchNorm / ReLU behind the layer: applied by whoever consumes `y`
  const float *W = nullptr, *b = nullptr, *gamma = nullptr, *beta = nullptr;
  float *rm = nullptr, *rv = nullptr;
  float* y = nullptr;                // raw (pre-BatchNorm) output [rows, ldy]
  long ldy = 0;
  float* Wpad = nullptr;             // input width no multiple of 4: zero-padded copy of W (null: W itself is fed to the kernels)
  long ldw = 0;                      // leading dimension of the weight actually fed to the kernels
  float *mean = nullptr, *rstd = nullptr, *s = nullptr, *t = nullptr;   // BatchNorm batch constants
  unsigned long long *slots = nullptr, *slots_bwd = nullptr;   // train mode: fixed-point slots of (sum x, sum x^2) / (sum dz, sum dz * xhat)
  float *dW = nullptr, *db = nullptr, *dgamma = nullptr, *dbeta = nullptr;
};

// Workspace carving in 256-byte steps; base may be null (size query).  Not `Carve` of spg_part.h: that one rounds the sizes too,
// and these entry points report `off` as their workspace bytes.
struct SpgCarver {
  char* base;
  size_t off = 0;
  explicit SpgCarver(void* b) : base((char*)b) {}
  template <typename T>
  T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? (T*)(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

// the C ABI hands every layer 6 parameter pointers {W, b, gamma, beta, running mean, running var} and 6 gradient slots of which
// the first 4 {dW, db, dgamma, dbeta} are written
inline int spg_dense_bind_params(SpgDenseLayer& l, const void* const* g) {
  l.W = (const float*)g[0]; l.b = (const float*)g[1]; l.gamma = (const float*)g[2]; l.beta = (const float*)g[3];
  l.rm = (float*)g[4]; l.rv = (float*)g[5];
  SPG_CHECK_ARG(l.W != nullptr, "missing layer weight");
  SPG_CHECK_ARG(!l.bn || (l.rm != nullptr && l.rv != nullptr), "missing BatchNorm running statistics");
  return 0;
}
inline void spg_dense_bind_grads(SpgDenseLayer& l, void* const* g) {
  l.dW = (float*)g[0]; l.db = (float*)g[1]; l.dgamma = (float*)g[2]; l.dbeta = (float*)g[3];
}

// ---- operands ----
inline SpgOperand spg_op_ident(const float* X, long ld) {
  SpgOperand o; memset(&o, 0, sizeof(o));
  o.mode = SPG_PRO_IDENT; o.X = X; o.ld = ld;
  return o;
}
// X * s + t (s may be null) and ReLU on the first n_affine channels
inline SpgOperand spg_op_affine(const float* X, long ld, int n_affine, const float* s, const float* t, int relu) {
  SpgOperand o; memset(&o, 0, sizeof(o));
  o.mode = SPG_PRO_AFFINE; o.X = X; o.ld = ld; o.c0 = s; o.c1 = t; o.relu = relu; o.n_affine = n_affine;
  return o;
}
// the output of `prod` as its consumer reads it: X [rows, ld] is prod.y or a view of it (the max-pooled rows)
inline SpgOperand spg_op_affine(const SpgDenseLayer& prod, const float* X, long ld) {
  return spg_op_affine(X, ld, prod.cout, prod.bn ? prod.s : nullptr, prod.bn ? prod.t : nullptr, prod.relu ? 1 : 0);
}
// the gradient dz wrt the BatchNorm OUTPUT of a layer with raw output y, read as the gradient wrt y; consts [4][C]
inline SpgOperand spg_op_bnbwd(const float* dz, const float* y, long ld, const float* consts, int C) {
  SpgOperand o; memset(&o, 0, sizeof(o));
  o.mode = SPG_PRO_BNBWD; o.X = dz; o.X2 = y; o.ld = ld;
  o.c0 = consts; o.c1 = consts + C; o.c2 = consts + 2 * C; o.c3 = consts + 3 * C;
  return o;
}
inline int spg_zero_bytes_async(void* p, size_t bytes, hipStream_t st) {
  if (p == nullptr || bytes == 0) return 0;
  hipError_t e = hipMemsetAsync(p, 0, bytes, st);
  if (e != hipSuccess) { spg_set_error("hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
  return 0;
}

// ---- BatchNorm hand-over ----
// May the train-mode statistics travel as slots from producer to consumer (no finalize launches)?  Not with synchronised BatchNorm
// (the ranks' all-reduce sits between producer and consumer), not beyond the slots' capacity; `contributions` = additions per
// channel of this rank's widest launch (4 per 32-row tile of PointNet's head: 4L * B; one per tile of the filter network).
// The backward asks again: the answer must not change between a forward and its backward.
inline bool spg_bn_fold_allowed(long contributions) {
  return !spg_sync_bn_active() && !spg_tune_get(SPG_TUNE_NO_BN_FOLD) && contributions * spg_slot_sync_world() <= SPG_FOLD_MAX_CONTRIBUTIONS;
}
// With slot-synchronised BatchNorm the statistics MUST travel through the slots: a rank that dropped to per-rank finalize
// statistics (its own row count beyond the slots' capacity, spg_tune key 10) would issue a different number of slot all-reduces
// than its peers -- a hang, or an unsynchronised model.  `has_bn`: a train-mode BatchNorm layer takes part.
inline int spg_bn_slot_sync_check(bool has_bn, bool fold, const char* msg) {
  SPG_CHECK_ARG(!(has_bn && spg_slot_sync_active()) || fold, msg);
  return 0;
}
// the statistics of `prod` (over `count` rows), finished in the prologue of the launch that consumes its output
inline SpgBnFold spg_fold_of(const SpgDenseLayer& prod, long count, int update_times, float momentum, float eps) {
  SpgBnFold f; memset(&f, 0, sizeof(f));
  f.slots = prod.slots; f.C = prod.cout; f.update_times = update_times; f.momentum = momentum; f.eps = eps;
  f.count = (double)count; f.gamma = prod.gamma; f.beta = prod.beta; f.rm = prod.rm; f.rv = prod.rv;
  f.mean = prod.mean; f.rstd = prod.rstd; f.s = prod.s; f.t = prod.t;
  return f;
}
// the BatchNorm-backward sums of `prod` (over `count` rows), finished by the next launch that applies `consts`
inline SpgBnFoldBwd spg_fold_bwd_of(const SpgDenseLayer& prod, long count, float* consts) {
  SpgBnFoldBwd f; memset(&f, 0, sizeof(f));
  f.slots = prod.slots_bwd; f.C = prod.cout; f.count = (double)count; f.s = prod.s; f.mean = prod.mean; f.rstd = prod.rstd;
  f.consts = consts; f.dgamma = prod.dgamma; f.dbeta = prod.dbeta;
  if (spg_slot_sync_active()) f.grad_mul = 1.0 / (double)spg_slot_sync_world();
  return f;
}

// ---- the two recipes ----
// How this pass makes batch statistics, and the scratch of the path without slots.
struct SpgDenseBn {
  bool training = false;
  bool fold = false;                 // spg_bn_fold_allowed (train mode only)
  int update_times = 1;
  float momentum = 0.f, eps = 0.f;
  float *stat = nullptr, *stat_cnt = nullptr;   // per-tile partials of the finalize path
  double* fin = nullptr;             // scratch of the sliced finalize (null: single-slice reduction)
  float* consts = nullptr;           // backward: [4][C] constants of the BatchNorm-backward operand
};

// Forward of layer `l` over M rows of `in`.  prod (may be null): the layer that produced `in`, whose statistics -- over
// prod_rows rows -- this launch finishes when they travel as slots.  grp (may be null): the caller's open scope, flushed behind
// the GEMM (before a finalize launch); null when the caller's stage flushes itself.  Eval-mode constants are the caller's.
inline int spg_dense_forward(const SpgDenseLayer& l, const SpgDenseLayer* prod, const SpgOperand& in, int M, long prod_rows,
                             const SpgDenseBn& bn, SpgGroupScope* grp, hipStream_t st) {
  SpgGemmParams g; memset(&g, 0, sizeof(g));
  g.a = in;
  if (prod != nullptr && prod->bn && bn.fold) g.fold = spg_fold_of(*prod, prod_rows, bn.update_times, bn.momentum, bn.eps);
  g.W = l.Wpad ? l.Wpad : l.W; g.ldw = l.ldw; g.bias = l.b; g.M = M; g.N = l.cout; g.K = l.cin; g.rows_per_tile = SPG_FC_ROWS;
  g.epi = SPG_EPI_FWD; g.Y = l.y; g.ldy = l.ldy;
  g.stat_cnt = bn.stat_cnt;
  if (l.bn && bn.fold) g.stat_slots = l.slots;
  else if (l.bn && bn.training) g.stat = bn.stat;
  const bool fin = l.bn && bn.training && !bn.fold;      // a finalize launch follows: the GEMM must not wait in a group
  int nparts = 0;
  {
    SpgGroupBypass direct(fin);
    SPG_TRY(spg_launch_gemm(g, st, &nparts));
  }
  if (grp != nullptr) SPG_TRY(grp->flush());
  if (fin)
    SPG_TRY(spg_launch_bn_finalize(bn.stat, bn.stat_cnt, nparts, M, l.cout, l.gamma, l.beta, l.rm, l.rv, bn.momentum, bn.eps,
                                   bn.update_times, l.mean, l.rstd, l.s, l.t, bn.fin, st));
  return 0;
}

// The data-gradient launch of a layer's backward: the gradient wrt the raw output of `prod`, the layer that produced its input.
struct SpgDenseDgrad {
  const SpgDenseLayer* prod = nullptr;   // null: the network's first layer, no data gradient
  float* out = nullptr;              // [M, ldout] gradient buffer
  long ldout = 0;
  const float* Yp = nullptr;         // raw output of prod as the forward consumed it [M, ldyp] (prod.y, or the max-pooled rows)
  long ldyp = 0;
  long count = 0;                    // rows behind prod's statistics
  long stat_rows = 0;                // rows this launch stands for in the slots' row count (0: M; SpgGemmParams::stat_rows)
  bool folds = false;                // the launch also finishes `pending` in its own prologue: needed when it shares a grouped launch
                                     // with the weight gradient, which otherwise runs first and finishes the constants
};

// Backward of layer `l` over M rows: {weight gradient with the bias riding along, bias zero or column sums, masked data gradient},
// then the finalize launch of prod's BatchNorm-backward sums or, when they travel as slots, the fold left in `pending`.
// cur: the gradient wrt l's raw output; in: l's forward input operand.  pending: in, the unfinished sums of cur's layer (or
// slots == null); out, those of d.prod.  grp (may be null): the caller's open scope, flushed behind the triple; null when the
// launches join a group the caller does not own (a rider stage) -- a data gradient followed by a finalize launch then bypasses it.
inline int spg_dense_backward(SpgReduceQueue& rq, const SpgDenseLayer& l, const SpgOperand& cur, const SpgOperand& in, int M,
                              const SpgDenseDgrad& d, const SpgDenseBn& bn, SpgBnFoldBwd& pending, SpgGroupScope* grp, hipStream_t st) {
  const SpgBnFoldBwd fold_l = pending;
  memset(&pending, 0, sizeof(pending));
  SpgWgradParams w; memset(&w, 0, sizeof(w));
  w.a = cur; w.b = in; w.M = M; w.N = l.cout; w.K = l.cin;
  w.fold = fold_l;
  // a bias without BatchNorm behind it: its gradient (column sums of `cur`, when that is an IDENT operand) rides along with the
  // weight gradient; a bias in front of train-mode BatchNorm has zero gradient
  const bool bias_rides = l.db != nullptr && !l.bn && cur.mode == SPG_PRO_IDENT;
  SPG_TRY(spg_queue_wgrad(rq, w, l.dW, st, bias_rides ? l.db : nullptr));
  if (l.db && !bias_rides) {
    if (l.bn) SPG_TRY(spg_group_zero(l.db, (size_t)l.cout, st));
    else SPG_TRY(spg_queue_colsum(rq, cur.X, cur.ld, M, l.cout, l.db, st));
  }
  if (d.prod == nullptr) return 0;
  const SpgDenseLayer& prod = *d.prod;
  SpgGemmParams g; memset(&g, 0, sizeof(g));
  g.a = cur; g.W = l.Wpad ? l.Wpad : l.W; g.ldw = l.ldw; g.w_red = 1;      // dz_prev = dy @ W, W read untransposed
  g.M = M; g.N = l.cin; g.K = l.cout; g.rows_per_tile = SPG_FC_ROWS;
  g.epi = SPG_EPI_BWD; g.Y = d.out; g.ldy = d.ldout; g.Yp = d.Yp; g.ldyp = d.ldyp;
  g.mask_relu = prod.relu ? 1 : 0; g.n_mask = prod.cout;
  const bool fin = prod.bn && !bn.fold;
  if (prod.bn) {
    g.ms = prod.s; g.mt = prod.t; g.mmean = prod.mean; g.mrstd = prod.rstd;
    if (bn.fold) { g.stat_slots = prod.slots_bwd; g.stat_rows = d.stat_rows; }
    else g.stat = bn.stat;
  }
  if (d.folds) g.fold_bwd = fold_l;
  int nparts = 0;
  {
    SpgGroupBypass direct(fin && grp == nullptr);
    SPG_TRY(spg_launch_gemm(g, st, &nparts));
  }
  if (grp != nullptr) SPG_TRY(grp->flush());
  // the statistics cover the producer's channels only (N = l.cin may be wider: concatenated global features)
  if (fin)
    SPG_TRY(spg_launch_bn_bwd_finalize(bn.stat, nparts, l.cin, d.count, prod.cout, prod.s, prod.mean, prod.rstd, bn.consts,
                                       prod.dgamma, prod.dbeta, bn.fin, st));
  else if (prod.bn) pending = spg_fold_bwd_of(prod, d.count, bn.consts);
  return 0;
}
