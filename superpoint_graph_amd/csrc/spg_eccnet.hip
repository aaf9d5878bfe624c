// RNN-ECC module (reference: RNNGraphConvModule.forward, learning/modules.py:152-183): filter-generating MLP on
// the superedge features (learning/graphnet.py:17-34), then nrepeats x {ECC aggregate, GRUCellEx}.
// Host-side orchestration of the forward / backward kernel sequences and the workspace layout.
//
// HBM layout: every per-node quantity that exists once per iteration is stored as [N][R+1][C]
// (states h^r, aggregates, and in the backward the gate gradients), so that "all iterations" is a plain
// row-major matrix with (R+1)*N rows for the deferred weight-gradient GEMMs, and a node's history is
// contiguous for the per-edge filter gradient (summed over the iterations in registers, written once).
#include "../../include/spg_hip.h"
#include "spg_ecc.h"
#include "spg_dense.h"
#include <memory>
#include <vector>

namespace {

struct Plan {
  spg_eccrnn_cfg cfg;
  int N = 0, E = 0, R = 0, nout = 0;
  int nc = 32;                  // state width: 32 (the kernels of spg_ecc.hip) or 8, 16, 64, 128 (spg_ecc_wide.hip)
  long ldS = 0;                 // (R+1)*nc
  int GW = 96;                  // gate rows of the cell: 3 nc (GRU) / 4 nc (LSTM)
  bool lstm = false;
  bool training = false;
  std::vector<SpgDenseLayer> F;
  bool fold = false;            // train mode: the BatchNorm statistics travel as fixed-point slots from producer to consumer GEMM
  bool px = false;              // the persistent (one launch for all iterations) GRU recurrence is applicable: rounds in `groups`
  SpgPxGroups groups;
  SpgGruParams gru;
  float *states = nullptr, *agg = nullptr, *stat = nullptr, *stat_cnt = nullptr;
  float* cells = nullptr;       // LSTM cell states c^r, laid out like `states`
  float* fsave = nullptr;       // persistent GRU recurrence, training: forward internals kept for the backward
  unsigned* fsave_tag = nullptr;
  float* cell_grads[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t bytes = 0;
};

int make_plan(const spg_eccrnn_cfg* cfg, int N, int E, int training, void* ws, const void* const* params, Plan& pl) {
  SPG_CHECK_ARG(cfg != nullptr && N > 0 && E >= 0, "cfg / N / E");
  const spg_eccrnn_cfg& c = *cfg;
  SPG_TRY(spg_wide_check(c.nc, c.matrix, "the fused RNN-ECC path"));
  SPG_CHECK_ARG(c.nrepeats >= 1, "nrepeats >= 1");
  SPG_CHECK_ARG(c.n_fnet >= 1 && c.n_fnet <= SPG_MAX_LAYERS, "n_fnet");
  SPG_CHECK_ARG(c.bnidx < c.n_fnet - 1 || c.bnidx < 0, "BatchNorm after the last filter layer is not supported");
  SPG_CHECK_ARG(c.cell == SPG_CELL_GRU || c.cell == SPG_CELL_LSTM, "cell must be 0 (GRU) or 1 (LSTM)");
  pl.cfg = c; pl.N = N; pl.E = E; pl.R = c.nrepeats; pl.training = training != 0;
  pl.lstm = c.cell == SPG_CELL_LSTM; pl.nc = c.nc; pl.GW = (pl.lstm ? 4 : 3) * pl.nc;
  pl.ldS = (long)(pl.R + 1) * pl.nc;
  pl.nout = c.matrix ? pl.nc * pl.nc : pl.nc;
  SPG_CHECK_ARG(c.fnet_widths[c.n_fnet] == pl.nout, "filter network output width must be nc*nc (matrix) or nc (vector)");
  SpgCarver cv(ws);
  pl.F.assign(c.n_fnet, SpgDenseLayer());
  int cmax = 4;
  for (int i = 0; i < c.n_fnet; ++i) {
    SpgDenseLayer& l = pl.F[i];
    l.cin = c.fnet_widths[i]; l.cout = c.fnet_widths[i + 1];
    l.bn = (c.bnidx == i); l.relu = i < c.n_fnet - 1;
    l.ldw = l.cin; l.ldy = l.cout;
    cmax = l.cout > cmax ? l.cout : cmax;
    if (params) SPG_TRY(spg_dense_bind_params(l, params + 6 * i));
    l.y = cv.take<float>((size_t)(E > 0 ? E : 1) * l.cout);
    if (l.bn) {
      l.mean = cv.take<float>(l.cout); l.rstd = cv.take<float>(l.cout);
      l.s = cv.take<float>(l.cout); l.t = cv.take<float>(l.cout);
      if (pl.training) {
        l.slots = cv.take<unsigned long long>(spg_fold_slot_words(l.cout));
        l.slots_bwd = cv.take<unsigned long long>(spg_fold_slot_words(l.cout));
      }
    }
  }
  memset(&pl.gru, 0, sizeof(pl.gru));
  if (params) {
    const void* const* g = params + 6 * c.n_fnet;
    pl.gru.w_ih = (const float*)g[0]; pl.gru.w_hh = (const float*)g[1];
    pl.gru.b_ih = (const float*)g[2]; pl.gru.b_hh = (const float*)g[3];
    pl.gru.w_ig = (const float*)g[4]; pl.gru.b_ig = (const float*)g[5];
    SPG_CHECK_ARG(pl.gru.w_ih && pl.gru.w_hh && pl.gru.b_ih && pl.gru.b_hh, "missing RNN cell parameters");
    SPG_CHECK_ARG(!c.ingate || (pl.gru.w_ig && pl.gru.b_ig), "missing input-gate parameters");
  }
  pl.gru.layernorm = c.layernorm; pl.gru.ingate = c.ingate;
  SPG_CHECK_ARG(pl.nc == 32 || (((uintptr_t)pl.gru.w_ih | (uintptr_t)pl.gru.w_hh | (uintptr_t)pl.gru.w_ig) & 15) == 0, "RNN cell weights must be 16-byte aligned");
  pl.states = cv.take<float>((size_t)N * pl.ldS);
  pl.agg = cv.take<float>((size_t)N * pl.ldS);
  if (pl.lstm) pl.cells = cv.take<float>((size_t)N * pl.ldS);
  // persistent GRU recurrence in training: the forward keeps the cell's internals of every (node, iteration) for the backward
  // (12 x 64 floats each: 31 MB per 1000 nodes x 10 iterations) instead of the backward recomputing them on its critical path
  pl.fsave = nullptr; pl.fsave_tag = nullptr;
  pl.px = pl.nc == 32 && !pl.lstm && c.n_parts >= 0 && c.n_parts <= SPG_MAX_PARTS && spg_px_plan_groups(N, c.n_parts, c.part_ptr, spg_tune_get(SPG_TUNE_NO_PERSIST_ECC), &pl.groups);
  // (more nodes than wavefronts -- one round above SPG_PX_MAX_NODES nodes: the backward recomputes the cell instead, spg_ecc.hip)
  if (pl.px && pl.training && !spg_px_groups_multi(pl.groups)) {
    pl.fsave_tag = cv.take<unsigned>(64);
    pl.fsave = cv.take<float>((size_t)N * pl.R * SPG_PX_SAVE_F * 64);
  }
  pl.stat = cv.take<float>((size_t)spg_cdiv(E > 0 ? E : 1, SPG_FC_ROWS) * 2 * cmax);
  pl.stat_cnt = cv.take<float>((size_t)spg_cdiv(E > 0 ? E : 1, SPG_FC_ROWS) + 64);
  pl.bytes = cv.off + 256;
  return 0;
}

SpgOperand fnet_input(const Plan& pl, int i, const float* edgefeats) {
  if (i == 0) return spg_op_ident(edgefeats, pl.F[0].cin);
  return spg_op_affine(pl.F[i - 1], pl.F[i - 1].y, pl.F[i - 1].ldy);
}

struct BwdScratch {
  float *G = nullptr, *dgi = nullptr, *dgh = nullptr, *dui = nullptr, *duh = nullptr, *dpre = nullptr, *xg = nullptr;
  float *dcdir = nullptr;
  float *dhdir = nullptr, *dWts = nullptr, *dzA = nullptr, *dzB = nullptr, *Wt = nullptr, *consts = nullptr;
  float *work = nullptr, *stat = nullptr;
  float* work2 = nullptr;   // reduction arena of the recurrent cell's parameter gradients (they may run on the side stream)
  size_t work_floats = 0, work2_floats = 0;
  size_t zero_bytes = 0;   // the leading region [G .. xg] must be zero-initialised
  size_t bytes = 0;
};

void carve_bwd(const Plan& pl, void* ws, BwdScratch& s) {
  SpgCarver cv(ws);
  const size_t rows = (size_t)pl.N * (pl.R + 1);
  const size_t nc = pl.nc;
  s.G = cv.take<float>(rows * nc);
  s.dgi = cv.take<float>(rows * pl.GW); s.dgh = cv.take<float>(rows * pl.GW);
  if (!pl.lstm) { s.dui = cv.take<float>(rows * pl.GW); s.duh = cv.take<float>(rows * pl.GW); }
  s.dpre = cv.take<float>(rows * nc); s.xg = cv.take<float>(rows * nc);
  s.zero_bytes = cv.off;
  s.dhdir = cv.take<float>((size_t)pl.N * nc);
  if (pl.lstm) s.dcdir = cv.take<float>((size_t)pl.N * nc);
  const size_t Er = pl.E > 0 ? pl.E : 1;
  s.dWts = cv.take<float>(Er * pl.nout);
  int cmax = 4;
  size_t wmax = 96 * 32, workmax = 16;
  for (const SpgDenseLayer& l : pl.F) {
    cmax = l.cout > cmax ? l.cout : cmax; cmax = l.cin > cmax ? l.cin : cmax;
    wmax = (size_t)l.cin * l.cout > wmax ? (size_t)l.cin * l.cout : wmax;
    workmax += spg_queue_layer_floats((long)Er, l.cout, l.cin);
  }
  // GRU: three weight gradients + three bias column sums over all (node, iteration) rows
  const size_t work2max = 16 + 3 * spg_queue_layer_floats((long)rows, pl.GW, pl.nc);
  int hmax = 4;   // widest hidden activation
  for (int i = 0; i + 1 < (int)pl.F.size(); ++i) hmax = pl.F[i].cout > hmax ? pl.F[i].cout : hmax;
  s.dzA = cv.take<float>(Er * hmax); s.dzB = cv.take<float>(Er * hmax);
  s.consts = cv.take<float>((size_t)4 * cmax);
  s.work = cv.take<float>(workmax); s.work_floats = workmax;
  s.work2 = cv.take<float>(work2max); s.work2_floats = work2max;
  s.stat = cv.take<float>((size_t)spg_cdiv(Er, SPG_FC_ROWS) * 2 * cmax);
  s.bytes = cv.off + 256;
}

}  // namespace

extern "C" size_t spg_eccrnn_workspace_bytes(const spg_eccrnn_cfg* cfg, int N, int E, int training) {
  Plan pl;
  if (make_plan(cfg, N, E, training, nullptr, nullptr, pl) != 0) return 0;
  return pl.bytes;
}

// train-mode BatchNorm of the filter network without finalize launches (spg_dense.h): one contribution per 32-edge tile.
// The slot-synchronised check needs an edge: an edge-less rank is refused by the forward's own checks.
static int fnet_fold(Plan& pl) {
  pl.fold = pl.training && spg_bn_fold_allowed(spg_cdiv(pl.E > 0 ? pl.E : 1, SPG_FC_ROWS));
  for (const SpgDenseLayer& l : pl.F)
    SPG_TRY(spg_bn_slot_sync_check(pl.training && pl.E > 0 && l.bn, pl.fold, "slot-synchronised BatchNorm needs the filter network's statistics slots (spg_tune key 10 off, edges within the slots' capacity on every rank)"));
  return 0;
}

// the BatchNorm side of one pass over the E edges (spg_dense.h)
static SpgDenseBn fnet_bn(const Plan& pl, int bn_update_times, float* stat, float* consts) {
  SpgDenseBn bn;
  bn.training = pl.training; bn.fold = pl.fold; bn.update_times = bn_update_times;
  bn.momentum = pl.cfg.bn_momentum; bn.eps = pl.cfg.bn_eps;
  bn.stat = stat; bn.stat_cnt = pl.stat_cnt; bn.consts = consts;
  return bn;
}

// ---- filter-generating network (once per forward, shared by all iterations): one stage per layer; each stage issues its
//      launches into the group that is open when it runs (spg_gemm.h) ----
static void fnet_forward_stages(const Plan& pl0, const float* edgefeats, int bn_update_times, std::vector<SpgStage>& out) {
  auto plan = std::make_shared<Plan>(pl0);
  for (int i = 0; i < (int)plan->F.size(); ++i) {
    out.push_back([plan, i, edgefeats, bn_update_times](hipStream_t st) -> int {
      const Plan& pl = *plan;
      const SpgDenseLayer& l = pl.F[i];
      if (i == 0 && pl.fold)                 // the statistics slots of both directions: cleared launches before their first use
        for (const SpgDenseLayer& f : pl.F)
          if (f.bn) {
            // BatchNorm behind the FIRST layer (--fnet_bnidx 0 is legal, learning/graphnet.py:17-37): this very stage's GEMM is the
            // slots' first producer, so a zero job in the same group would race with it -- clear them in stream order instead
            if (&f == &pl.F[0]) SPG_TRY(spg_zero_bytes_async(f.slots, sizeof(float) * 2 * spg_fold_slot_words(f.cout), st));
            else SPG_TRY(spg_group_zero(reinterpret_cast<float*>(f.slots), 2 * spg_fold_slot_words(f.cout), st));
            SPG_TRY(spg_group_zero(reinterpret_cast<float*>(f.slots_bwd), 2 * spg_fold_slot_words(f.cout), st));
          }
      SPG_TRY(spg_dense_forward(l, i > 0 ? &pl.F[i - 1] : nullptr, fnet_input(pl, i, edgefeats), pl.E, pl.E,
                                fnet_bn(pl, bn_update_times, pl.stat, nullptr), nullptr, st));
      if (l.bn && !pl.training) SPG_TRY(spg_launch_bn_eval(l.cout, l.gamma, l.beta, l.rm, l.rv, pl.cfg.bn_eps, l.s, l.t, st));
      return 0;
    });
  }
}

// head (optional, spg_train_step): classifier + cross entropy behind the last iteration, inside the persistent launch
// (SpgEccHead, spg_ecc.h); *head_done says whether that launch took it -- the caller runs the separate launches otherwise
static int eccrnn_recurrent_forward(Plan& pl, const void* graph_ws, const float* h0, float* out, hipStream_t st,
                                    const SpgEccScatter* sc, const SpgEccHead* head = nullptr, bool* head_done = nullptr) {
  if (head_done != nullptr) *head_done = false;
  const int N = pl.N, E = pl.E;
  SpgGraph gr = spg_graph_view(graph_ws, N, E);
  const int64_t* h0_rows = nullptr;
  if (sc != nullptr) { h0 = sc->emb; h0_rows = sc->slot_of_row; }      // the embedding scatter read in place (persistent launch)
  if (pl.px) {      // GRU: all iterations in one dataflow-synchronised launch, whole scenes in rounds of <= 2048 nodes (spg_ecc.hip)
    SpgEccPersistFwd q; memset(&q, 0, sizeof(q));
    q.groups = pl.groups;
    q.g = gr; q.W = pl.F.back().y; q.matrix = pl.cfg.matrix; q.R = pl.R; q.h0 = h0; q.h0_rows = h0_rows;
    q.states = pl.states; q.ldS = pl.ldS; q.agg = pl.training ? pl.agg : nullptr;
    q.out = out; q.cat_all = pl.cfg.cat_all; q.ldo = pl.cfg.cat_all ? pl.ldS : 32; q.gru = pl.gru;
    q.fsave = pl.fsave; q.fsave_tag = pl.fsave_tag;
    const bool with_head = head != nullptr && head_done != nullptr && !spg_px_groups_multi(pl.groups) && head->nin == (pl.cfg.cat_all ? 32 * (pl.R + 1) : 32) &&
                           head->C <= SPG_PX_HEAD_MAXC && spg_px_head_lds_bytes(*head) <= SPG_PX_HEAD_LDS;
    if (with_head) q.head = *head;
    int err = 0;
    if (spg_launch_ecc_persist_fwd(q, st, &err)) {
      if (with_head && err == 0) *head_done = true;
      return err;
    }
  }
  const int nc = pl.nc;
  if (sc != nullptr) {      // per-iteration launches read a materialised descriptor matrix
    SPG_TRY(spg_gather_rows(sc->emb, nc, sc->slot_of_row, N, nc, sc->desc, nc, (void*)st));
    h0 = sc->desc;
  }
  if (pl.fsave_tag != nullptr) SPG_TRY(spg_zero_bytes_async(pl.fsave_tag, sizeof(unsigned), st));      // per-iteration path: nothing was kept
  SPG_TRY(spg_launch_copy2d(h0, nc, pl.states, pl.ldS, N, nc, st));
  for (int r = 0; r < pl.R; ++r) {
    SpgEccStepFwd p; memset(&p, 0, sizeof(p));
    p.g = gr; p.W = pl.F.back().y; p.matrix = pl.cfg.matrix;
    p.hin = pl.states + (size_t)r * nc; p.hout = pl.states + (size_t)(r + 1) * nc; p.ld = pl.ldS;
    p.agg_save = pl.training ? pl.agg + (size_t)r * nc : nullptr; p.ldagg = pl.ldS;
    p.do_gru = 1; p.gru = pl.gru; p.cell = pl.cfg.cell;
    if (pl.lstm) { p.cin = r > 0 ? pl.cells + (size_t)r * nc : nullptr; p.cout = pl.cells + (size_t)(r + 1) * nc; }
    SPG_TRY(spg_ecc_step_fwd(p, nc, st));
  }
  if (pl.cfg.cat_all) SPG_TRY(spg_launch_copy2d(pl.states, pl.ldS, out, pl.ldS, N, (int)pl.ldS, st));
  else SPG_TRY(spg_launch_copy2d(pl.states + (size_t)pl.R * nc, pl.ldS, out, nc, N, nc, st));
  return 0;
}

// phase 0: the whole forward; phase 1: register the filter network's layers as riders (spg_gemm.h) and return -- they leave with
// the caller's next grouped launches; phase 2: the recurrent part only (the caller has drained the riders)
int spg_eccrnn_forward_phase(const spg_eccrnn_cfg* cfg, int N, int E, const void* graph_ws, const float* h0, const float* edgefeats,
                             const void* const* params, float* out, void* workspace, int training, int bn_update_times, void* stream,
                             int phase, const SpgEccScatter* sc, const SpgEccHead* head, bool* head_done) {
  SPG_CHECK_ARG(graph_ws && params && workspace && (phase == 1 || ((h0 || sc) && out)), "null pointer");
  SPG_CHECK_ARG(E == 0 || edgefeats != nullptr, "edgefeats");
  hipStream_t st = (hipStream_t)stream;
  Plan pl;
  SPG_TRY(make_plan(cfg, N, E, training, workspace, params, pl));
  SPG_TRY(fnet_fold(pl));
  if (E == 0 && pl.training && spg_slot_sync_active())
    for (const SpgDenseLayer& l : pl.F) SPG_CHECK_ARG(!l.bn, "slot-synchronised BatchNorm: a rank with an edge-less batch cannot take part in the filter-network statistics");
  if (E == 0 && pl.training && spg_sync_bn_active())
    for (const SpgDenseLayer& l : pl.F)      // the other ranks enter the layer's all-reduce: skipping it here would hang the job
      SPG_CHECK_ARG(!l.bn, "synchronised BatchNorm: a rank with an edge-less batch cannot take part in the filter-network statistics");
  if (phase != 2 && E > 0) {
    std::vector<SpgStage> stages;
    fnet_forward_stages(pl, edgefeats, bn_update_times, stages);
    if (phase == 1) {
      for (SpgStage& s : stages) spg_riders_push(std::move(s));
      return 0;
    }
    for (SpgStage& s : stages) {      // on their own: every layer is a launch (a group of one, + the slot clearing)
      SpgGroupScope grp(st);
      SPG_TRY(s(st));
      SPG_TRY(grp.flush());
    }
  }
  if (phase == 1) return 0;
  return eccrnn_recurrent_forward(pl, graph_ws, h0, out, st, sc, head, head_done);
}

extern "C" int spg_eccrnn_forward(const spg_eccrnn_cfg* cfg, int N, int E, const void* graph_ws, const float* h0,
                                  const float* edgefeats, const void* const* params, float* out, void* workspace,
                                  int training, int bn_update_times, void* stream) {
  return spg_eccrnn_forward_phase(cfg, N, E, graph_ws, h0, edgefeats, params, out, workspace, training, bn_update_times, stream, 0, nullptr, nullptr, nullptr);
}

extern "C" long spg_eccrnn_debug_offset(const spg_eccrnn_cfg* cfg, int N, int E, int training, int layer, int what) {
  Plan pl;
  char* fake = (char*)(uintptr_t)4096;
  if (make_plan(cfg, N, E, training, fake, nullptr, pl) != 0 || layer < 0 || layer >= (int)pl.F.size()) return -1;
  const SpgDenseLayer& l = pl.F[layer];
  const void* p = what == 0 ? (const void*)l.y : what == 1 ? l.s : what == 2 ? l.t : what == 3 ? l.mean : what == 4 ? l.rstd : nullptr;
  return p == nullptr ? -1 : (long)((const char*)p - fake);
}

extern "C" size_t spg_eccrnn_bwd_workspace_bytes(const spg_eccrnn_cfg* cfg, int N, int E) {
  Plan pl;
  if (make_plan(cfg, N, E, 1, nullptr, nullptr, pl) != 0) return 0;
  BwdScratch s;
  carve_bwd(pl, nullptr, s);
  return s.bytes;
}

// everything the backward's stages share (they may run after spg_eccrnn_backward_phase has returned: as riders)
namespace {
struct BwdCtx {
  Plan pl;
  BwdScratch s;
  SpgReduceQueue rq, rq2;
  SpgGraph gr;
  const float* edgefeats = nullptr;
  SpgOperand cur;
  int flip = 0;
  SpgBnFoldBwd pending;       // set by a data-gradient stage, finished by the next layer's launches (fold path)
};

// the tail of the backward: {cell parameter gradients + per-edge filter gradient}, then one stage per filter-network layer
// ({weight gradient, bias column sums, data gradient}: mutually independent), then the hand-over of the split partials
void eccrnn_backward_tail_stages(std::shared_ptr<BwdCtx> c, std::vector<SpgStage>& out, SpgStage extra_leaf) {
  // the recurrent cell's parameter gradients: three weight gradients + three bias column sums over all (node, iteration) rows.
  // A LEAF -- nothing in the chain below depends on them -- so they do not sit in front of the filter network's chain: they
  // leave with the stage of filter layer n-2 (their ~2000 small workgroups next to that layer's few)
  auto cell_grads = [c](hipStream_t st) -> int {
    Plan& pl = c->pl; BwdScratch& s = c->s;
    const int R = pl.R, GW = pl.GW, rows = pl.N * (R + 1);
    SpgWgradParams w; memset(&w, 0, sizeof(w));
    const int nc = pl.nc;
    w.a = spg_op_ident(s.dgi, GW); w.b = spg_op_ident(s.xg, nc); w.M = rows; w.N = GW; w.K = nc;
    SPG_TRY(spg_queue_wgrad(c->rq2, w, pl.cell_grads[0], st));
    w.a = spg_op_ident(s.dgh, GW); w.b = spg_op_ident(pl.states, nc);
    SPG_TRY(spg_queue_wgrad(c->rq2, w, pl.cell_grads[1], st));
    // GRU: the biases are added behind the row normalisation; LSTM: in front of it
    SPG_TRY(spg_queue_colsum(c->rq2, pl.lstm ? s.dgi : s.dui, GW, rows, GW, pl.cell_grads[2], st));
    SPG_TRY(spg_queue_colsum(c->rq2, pl.lstm ? s.dgh : s.duh, GW, rows, GW, pl.cell_grads[3], st));
    if (pl.cfg.ingate) {
      w.a = spg_op_ident(s.dpre, nc); w.b = spg_op_ident(pl.states, nc); w.N = nc;
      // the input gate's bias gradient = column sums of dpre: as their own small job, not riding along with the weight
      // gradient -- the body that carries them needs more than 128 registers and would push the whole group (2700 small
      // workgroups) to the 2-workgroups-per-CU build of the grouped kernel (spg_gemm.hip)
      SPG_TRY(spg_queue_wgrad(c->rq2, w, pl.cell_grads[4], st));
      SPG_TRY(spg_queue_colsum(c->rq2, s.dpre, nc, rows, nc, pl.cell_grads[5], st));
    }
    return 0;
  };
  const int nF = (int)c->pl.F.size();
  const int leaf_with = c->pl.E > 0 && nF >= 2 ? nF - 2 : -1;      // the filter-layer stage the cell gradients travel with (-1: the first stage)
  // the caller's own leaf (spg_train_step: the classifier's parameter gradients -- a body of the 2-per-CU build of the grouped
  // kernel): with the LAST filter layer's stage, which needs that build anyway (in the first stage it pushed the per-edge filter
  // gradient's 1300 small workgroups off the 4-per-CU build: 14.5 -> 24.6 us; measured: +10 us whichever stage carries it)
  const int extra_with = c->pl.E > 0 && nF >= 1 ? nF - 1 : -1;
  out.push_back([c, cell_grads, leaf_with, extra_leaf, extra_with](hipStream_t st) -> int {
    Plan& pl = c->pl; BwdScratch& s = c->s;
    const int R = pl.R;
    const long ldS = pl.ldS;
    if (extra_leaf && extra_with < 0) SPG_TRY(extra_leaf(st));
    if (leaf_with < 0) SPG_TRY(cell_grads(st));
    if (pl.E == 0) {   // no edges: the filter network received no gradient
      for (SpgDenseLayer& l : pl.F) {
        SPG_TRY(spg_group_zero(l.dW, (size_t)l.cin * l.cout, st));
        SPG_TRY(spg_group_zero(l.db, (size_t)l.cout, st));
        SPG_TRY(spg_group_zero(l.dgamma, (size_t)l.cout, st));
        SPG_TRY(spg_group_zero(l.dbeta, (size_t)l.cout, st));
      }
      return 0;
    }
    // per-edge filter gradients (sum over the iterations): the head of the filter network's chain
    // (32: a job of the open grouped launch; the other widths: their own launch, in stream order)
    SPG_TRY(spg_ecc_edge_wgrad(c->gr, pl.cfg.matrix, pl.nc, pl.states, ldS, s.G, ldS, R, s.dWts, st));
    c->cur = spg_op_ident(s.dWts, pl.nout);
    return 0;
  });
  for (int i = (int)c->pl.F.size() - 1; i >= 0 && c->pl.E > 0; --i) {
    out.push_back([c, i, cell_grads, leaf_with, extra_leaf, extra_with](hipStream_t st) -> int {
      Plan& pl = c->pl; BwdScratch& s = c->s;
      const int E = pl.E;
      SpgDenseLayer& l = pl.F[i];
      if (i == leaf_with) SPG_TRY(cell_grads(st));
      if (extra_leaf && i == extra_with) SPG_TRY(extra_leaf(st));
      const SpgOperand cur = c->cur;
      SpgDenseDgrad d;
      if (i > 0) {
        float* dzb[2] = {s.dzA, s.dzB};
        d.prod = &pl.F[i - 1]; d.out = dzb[c->flip]; d.ldout = l.cin; d.Yp = d.prod->y; d.ldyp = d.prod->ldy; d.count = E;
        d.folds = true;      // (the weight gradient of this layer may run in the same grouped launch: both finish the constants)
        c->flip ^= 1;
      }
      SPG_TRY(spg_dense_backward(c->rq, l, cur, fnet_input(pl, i, c->edgefeats), E, d, fnet_bn(pl, 1, s.stat, s.consts), c->pending, nullptr, st));
      if (i > 0) c->cur = d.prod->bn ? spg_op_bnbwd(d.out, d.prod->y, d.prod->ldy, s.consts, d.prod->cout) : spg_op_ident(d.out, l.cin);
      return 0;
    });
  }
  // the split partials of all weight / bias gradients: handed to the NEXT batched reduction of this thread (spg_gemm.h:
  // spg_reduce_defer) -- PointNet's, when this chain rides next to its backward -- or summed by the caller's own flush
  out.push_back([c](hipStream_t st) -> int {
    for (int j = 0; j < c->rq2.njobs; ++j) spg_reduce_defer(c->rq2.jobs[j]);
    for (int j = 0; j < c->rq.njobs; ++j) spg_reduce_defer(c->rq.jobs[j]);
    c->rq.njobs = 0; c->rq2.njobs = 0;
    return 0;
  });
}
}  // namespace

// phase 0: the whole backward; phase 1: back-propagation through the recurrence (-> grad_h0), the tail (cell and filter-network
// parameter gradients) is registered as riders (spg_gemm.h): the caller lets them travel next to its next launches and MUST
// call spg_riders_drain + spg_flush_deferred_reduce before the gradients are consumed or the workspaces released
int spg_eccrnn_backward_phase(const spg_eccrnn_cfg* cfg, int N, int E, const void* graph_ws, const float* edgefeats,
                              const void* const* params, const float* grad_out, float* grad_h0, void* const* grads,
                              void* workspace, void* bwd_workspace, void* stream, int phase, const SpgEccScatter* sc,
                              SpgStage extra_leaf, const SpgEccHead* head) {
  SPG_CHECK_ARG(graph_ws && params && grad_out && grad_h0 && grads && workspace && bwd_workspace, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (phase == 0) spg_reduce_deferred_clear();      // (nothing may be left over from a call that failed half-way)
  auto c = std::make_shared<BwdCtx>();
  Plan& pl = c->pl;
  SPG_TRY(make_plan(cfg, N, E, 1, workspace, params, pl));
  SPG_TRY(fnet_fold(pl));
  for (size_t i = 0; i < pl.F.size(); ++i) spg_dense_bind_grads(pl.F[i], grads + 6 * i);
  for (int k = 0; k < 6; ++k) pl.cell_grads[k] = (float*)grads[6 * pl.F.size() + k];
  BwdScratch& s = c->s;
  carve_bwd(pl, bwd_workspace, s);
  c->rq.arena = s.work; c->rq.arena_floats = s.work_floats;
  c->rq2.arena = s.work2; c->rq2.arena_floats = s.work2_floats;
  c->gr = spg_graph_view(graph_ws, N, E);
  c->edgefeats = edgefeats;
  memset(&c->cur, 0, sizeof(c->cur));
  memset(&c->pending, 0, sizeof(c->pending));
  SpgGraph& gr = c->gr;
  const int R = pl.R;
  const int GW = pl.GW, nc = pl.nc;
  const long ldS = pl.ldS, ld96 = (long)(R + 1) * GW;
  // ---- back-propagation through the R iterations ----
  bool persistent = false;
  if (pl.px) {      // GRU: one dataflow-synchronised launch for all iterations (spg_ecc.hip)
    SpgEccPersistBwd q; memset(&q, 0, sizeof(q));
    q.groups = pl.groups;
    q.g = gr; q.W = pl.F.back().y; q.matrix = pl.cfg.matrix; q.R = R; q.cat_all = pl.cfg.cat_all;
    q.grad_out = grad_out; q.ldgo = pl.cfg.cat_all ? ldS : 32;
    q.states = pl.states; q.ldS = ldS; q.agg = pl.agg; q.G = s.G;
    q.dgi = s.dgi; q.dgh = s.dgh; q.dui = s.dui; q.duh = s.duh; q.ld96 = ld96;
    q.dpre = s.dpre; q.xg = s.xg; q.ld32 = ldS; q.gx = grad_h0; q.gru = pl.gru;
    if (sc != nullptr) { q.gx = sc->grad_emb; q.gx_rows = sc->slot_of_row; }      // the gradient gather written in place
    q.fsave = pl.fsave; q.fsave_tag = pl.fsave_tag;
    if (head != nullptr) q.head = *head;      // the head the forward launch ran: this launch sums its loss
    int err = 0;
    bool wgrad_done = false;
    persistent = spg_launch_ecc_persist_bwd(q, st, &err, head != nullptr ? &wgrad_done : nullptr);      // writes every row of [G .. xg] itself (slot R: zeros)
    if (err != 0) return err;
    if (wgrad_done) extra_leaf = SpgStage();      // the launch formed the classifier's parameter gradients on idle CUs
  }
  if (head != nullptr && !persistent)      // (the per-iteration fallback: the loss from the head's logits, as its own launch)
    SPG_TRY(spg_cross_entropy_fwd(head->logits, head->target, head->class_weight, N, head->C, head->ignore_index, head->reduction_mean,
                                  head->loss, head->lse, head->wsum, stream));
  if (!persistent) SPG_TRY(spg_zero_bytes_async(bwd_workspace, s.zero_bytes, st));
  for (int r = R - 1; r >= 0 && !persistent; --r) {
    SpgEccStepBwd p; memset(&p, 0, sizeof(p));
    p.g = gr; p.W = pl.F.back().y; p.matrix = pl.cfg.matrix;
    if (pl.cfg.cat_all) { p.dcat = grad_out + (size_t)(r + 1) * nc; p.ldc = ldS; }
    else if (r == R - 1) { p.dcat = grad_out; p.ldc = nc; }
    p.Gnext = r < R - 1 ? s.G + (size_t)(r + 1) * nc : nullptr; p.ldg = ldS;
    p.dhdir = s.dhdir; p.use_dhdir = r < R - 1;
    p.hin = pl.states + (size_t)r * nc; p.ld = ldS;
    p.agg = pl.agg + (size_t)r * nc; p.ldagg = ldS;
    p.Gcur = s.G + (size_t)r * nc;
    p.dgi = s.dgi + (size_t)r * GW; p.dgh = s.dgh + (size_t)r * GW; p.ld96 = ld96;
    if (!pl.lstm) { p.dui = s.dui + (size_t)r * GW; p.duh = s.duh + (size_t)r * GW; }
    p.dpre = s.dpre + (size_t)r * nc; p.xg = s.xg + (size_t)r * nc; p.ld32 = ldS;
    p.gru = pl.gru; p.cell = pl.cfg.cell;
    if (pl.lstm) { p.cin = r > 0 ? pl.cells + (size_t)r * nc : nullptr; p.dcdir = s.dcdir; p.use_dcdir = r < R - 1; }
    SPG_TRY(spg_ecc_step_bwd(p, nc, st));
  }
  if (!persistent) {
    SpgEccStepBwd p; memset(&p, 0, sizeof(p));
    p.g = gr; p.W = pl.F.back().y; p.matrix = pl.cfg.matrix;
    if (pl.cfg.cat_all) { p.dcat = grad_out; p.ldc = ldS; }
    p.Gnext = s.G; p.ldg = ldS; p.dhdir = s.dhdir; p.use_dhdir = 1; p.gx = grad_h0; p.final_only = 1;
    p.gru = pl.gru; p.cell = pl.cfg.cell;
    SPG_TRY(spg_ecc_step_bwd(p, nc, st));
  }
  if (sc != nullptr && !persistent)       // per-iteration launches wrote grad_h0 [N, nc]: gather the embeddable rows
    SPG_TRY(spg_gather_rows(grad_h0, nc, sc->idx_valid, sc->B, nc, sc->grad_emb, nc, stream));
  // ---- the tail: nothing below depends on it, it depends on nothing but the recurrence's outputs ----
  std::vector<SpgStage> stages;
  eccrnn_backward_tail_stages(c, stages, std::move(extra_leaf));
  if (phase == 1) {
    for (SpgStage& sg : stages) spg_riders_push(std::move(sg));
    return 0;
  }
  for (SpgStage& sg : stages) {      // on their own: one grouped launch per stage
    SpgGroupScope grp(st);
    SPG_TRY(sg(st));
    SPG_TRY(grp.flush());
  }
  return spg_flush_deferred_reduce(st);     // ONE launch sums the split partials of all weight / bias gradients
}

extern "C" int spg_eccrnn_backward(const spg_eccrnn_cfg* cfg, int N, int E, const void* graph_ws, const float* edgefeats,
                                   const void* const* params, const float* grad_out, float* grad_h0, void* const* grads,
                                   void* workspace, void* bwd_workspace, void* stream) {
  return spg_eccrnn_backward_phase(cfg, N, E, graph_ws, edgefeats, params, grad_out, grad_h0, grads, workspace, bwd_workspace, stream, 0, nullptr, SpgStage(), nullptr);
}
