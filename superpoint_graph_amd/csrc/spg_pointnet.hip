// PointNet superpoint embedder on the fused row-GEMM kernels: host-side orchestration (kernel sequence,
// workspace layout) of the forward and backward passes.  Reference: learning/pointnet.py:16-133
// (STNkD, PointNet); CloudEmbedder's recompute-in-backward (pointnet.py:160-176) is replaced by keeping
// the raw layer outputs in HBM (288 GB per GPU), the BatchNorm running statistics are updated as many
// times as the reference's double forward would.
//
// Data layout in HBM
//   clouds         [B, nfeat, P]    as the loader produces them (channel-major per superpoint)
//   y_l            [B*P, C_l]       raw (pre-BatchNorm) output of 1x1-conv layer l, row = b*P + p
//   y_fc           [B, C]           raw output of an FC layer
//   BatchNorm(+ReLU) is applied by the CONSUMER while staging its tile into LDS (scale s, shift t per
//   channel), so normalised activations are never written.
//   The max-pool over the points is fused into the epilogue of the last conv (per-superpoint max AND
//   min of the raw output: after the batch statistics are known, sign(s) decides which one is the
//   max of the normalised value -- BatchNorm is monotone per channel).
//   More than 128 points per superpoint (spg_segments.h): the convolutions run on Bc = B * S pseudo-superpoints of Pc = P / S points
//   in the same row space (row b*P + p = (b*S + s)*Pc + p'); the clouds and transforms are copied into that view, the epilogue's
//   per-segment extrema are merged into pooled / aidx [B, ldpool] (winner = point index in the superpoint), and the backward expands
//   the pooled gradient back to per-segment rows.  Up to 128 points S = 1 and nothing of this is launched or allocated.
#include "../../include/spg_hip.h"
#include "spg_ecc.h"
#include "spg_dense.h"
#include "spg_narrow.h"
#include "spg_segments.h"
#include <limits.h>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace {
// Which Gram-slot arrays (one per workspace and segment: the device address is the key) the LAST training forward filled
// (spg_narrow.hip's one-pass first layers).  The backward of the first convolution takes its one-pass form only then: it used to
// re-evaluate the forward's predicates (spg_tune keys 17 / 18, the fold, the shapes) -- had they changed in between (A/B tooling
// toggling spg_tune), it would have read zeroed slots and written a wrong dW1 / dT without any error.
std::mutex g_gram_mu;
std::unordered_map<const void*, bool> g_gram_filled;
void gram_record(const void* slots, bool filled) { std::lock_guard<std::mutex> lock(g_gram_mu); g_gram_filled[slots] = filled; }
bool gram_recorded(const void* slots) {
  std::lock_guard<std::mutex> lock(g_gram_mu);
  auto it = g_gram_filled.find(slots);
  return it != g_gram_filled.end() && it->second;
}

struct Layer : SpgDenseLayer {
  bool conv = false;            // rows = points (B*P) instead of superpoints (B)
  float* Wpack = nullptr;       // conv layers, inference: weights in MFMA operand order (spg_convstack.hip)
  void *Wb_f = nullptr, *Wb_t = nullptr;   // conv layers with whole reduction chunks: bf16 hi/lo copies of W for the opt-in bf16 MFMA
                                // modes (spg_launch_split_weights): forward orientation [2][cout][cin], transposed [2][cin][cout]
};

struct Segment {           // convs (BN+ReLU each) -> max-pool (+concat) -> fcs (BN+ReLU each, last one plain)
  std::vector<int> convs, fcs;
  float* pooled = nullptr;  // [B, C_lastconv + nextra] selected raw max / min (+ concatenated global features)
  long ldpool = 0;
  int* aidx = nullptr;      // [B, C_lastconv]
  int nextra = 0;
  const float* extra = nullptr;
  unsigned long long* gram = nullptr;   // train mode: fixed-point slots of the Gram matrix of the segment's input (spg_narrow.h)
  // npts > 128 (spg_segments.h): what the pooled convolution writes per pseudo-superpoint, [Bc, ldseg]; pooled / aidx are merged from them
  float* spool = nullptr;
  int* sidx = nullptr;
  long ldseg = 0;
};

struct Plan {
  spg_pointnet_cfg cfg;
  int B = 0, P = 0;
  long M = 0;
  // the convolutions' view: Bc = B * S pseudo-superpoints of Pc points (spg_segments.h); S = 1, Bc = B, Pc = P up to 128 points
  int S = 1, Bc = 0, Pc = 0;
  float* seg_clouds = nullptr;   // S > 1: [Bc, nfeat, Pc] copy of the clouds
  float* seg_T = nullptr;        // S > 1: [Bc, 4] rows of the transform (inner STN's projection or external)
  bool training = false;
  std::vector<Layer> L;
  Segment stn, main;
  bool has_stn = false;
  // shared scratch
  float *stat = nullptr, *stat_cnt = nullptr, *pmax = nullptr, *pmin = nullptr;
  double* fin = nullptr;    // scratch of the sliced BatchNorm finalize
  int *imax = nullptr, *imin = nullptr;
  unsigned long long* slots_all = nullptr;  // all layers' statistics slots, one region (cleared by one memset per forward)
  size_t slots_words = 0;
  bool fold = false;        // train mode: BatchNorm statistics are finished by the consuming GEMM instead of a finalize launch
  bool pads_done = false;   // the zero-padded weight copies of this forward have been issued
  size_t bytes = 0;
};

int num_layers(const spg_pointnet_cfg& c) {
  return (c.nfeat_stn > 0 ? c.n_stn_conv + c.n_stn_fc + 1 : 0) + c.n_conv + c.n_fc;
}

// builds the layer table and carves the forward workspace (base may be null: size query)
int make_plan(const spg_pointnet_cfg* cfg, int B, int training, void* ws, const void* const* params, float* emb,
              Plan& pl) {
  SPG_CHECK_ARG(cfg != nullptr && B > 0, "cfg / B");
  const spg_pointnet_cfg& c = *cfg;
  int Ps = 0, S = 0;
  if (!spg_segment_plan(c.npts, &Ps, &S)) {
    spg_set_error("PointNet: npts = %d is not supported: " SPG_SEG_RULE, c.npts);
    return -2;
  }
  SPG_CHECK_ARG(c.n_conv >= 1 && c.n_fc >= 1 && c.n_conv <= SPG_MAX_LAYERS && c.n_fc <= SPG_MAX_LAYERS, "layer counts");
  SPG_CHECK_ARG(c.last_ac == 0, "last_ac=True is not supported");
  SPG_CHECK_ARG(c.nfeat_stn == 0 || (c.nfeat_stn >= 2 && c.nfeat_stn <= c.nfeat && c.n_stn_conv >= 1 && c.n_stn_fc >= 1),
                "STN configuration");
  SPG_CHECK_ARG(c.nfeat >= 1 && c.nfeat <= 32, "nfeat must be <= 32");
  pl.cfg = c; pl.B = B; pl.P = c.npts; pl.M = (long)B * c.npts; pl.training = training != 0;
  pl.S = S; pl.Pc = Ps; pl.Bc = B * S;
  SPG_CHECK_ARG((long)B * c.npts < (1L << 31), "B * npts");
  pl.has_stn = c.nfeat_stn > 0;
  pl.L.clear();
  auto add = [&](int cin, int cout, bool bn, bool conv) {
    Layer l; l.cin = cin; l.cout = cout; l.bn = bn; l.relu = bn; l.conv = conv;      // (every BatchNorm here is followed by a ReLU)
    pl.L.push_back(l);
    return (int)pl.L.size() - 1;
  };
  pl.stn = Segment(); pl.main = Segment();
  if (pl.has_stn) {
    for (int i = 0; i < c.n_stn_conv; ++i) pl.stn.convs.push_back(add(i ? c.stn_conv[i - 1] : c.nfeat_stn, c.stn_conv[i], true, true));
    for (int i = 0; i < c.n_stn_fc; ++i)
      pl.stn.fcs.push_back(add(i ? c.stn_fc[i - 1] : c.stn_conv[c.n_stn_conv - 1], c.stn_fc[i], true, false));
    pl.stn.fcs.push_back(add(c.stn_fc[c.n_stn_fc - 1], 4, false, false));   // proj
  }
  for (int i = 0; i < c.n_conv; ++i) pl.main.convs.push_back(add(i ? c.conv[i - 1] : c.nfeat, c.conv[i], true, true));
  for (int i = 0; i < c.n_fc; ++i)
    pl.main.fcs.push_back(add(i ? c.fc[i - 1] : c.conv[c.n_conv - 1] + c.nfeat_global, c.fc[i], i < c.n_fc - 1, false));
  pl.main.nextra = c.nfeat_global;

  SpgCarver cv(ws);
  int cmax = 4;
  for (size_t i = 0; i < pl.L.size(); ++i) {
    Layer& l = pl.L[i];
    if (params) SPG_TRY(spg_dense_bind_params(l, params + 6 * i));
    cmax = l.cout > cmax ? l.cout : cmax;
    if (l.bn) {
      l.mean = cv.take<float>(l.cout); l.rstd = cv.take<float>(l.cout);
      l.s = cv.take<float>(l.cout); l.t = cv.take<float>(l.cout);
    }
    l.ldw = l.cin;
    if (!l.conv && (l.cin & 3) != 0) {     // e.g. 256 pooled channels + 1 diameter = 257
      l.ldw = (l.cin + 3) & ~3;
      l.Wpad = cv.take<float>((size_t)l.cout * l.ldw);
    }
    // training, first convolution of the main segment behind an STN: its data gradient wrt the transformed xy reads the weight
    // untransposed [cout][cin]; with cin no multiple of 4 (14, 11) a zero-padded copy keeps it on the vector staging path
    if (l.conv && pl.training && pl.has_stn && (int)i == (pl.has_stn ? c.n_stn_conv + c.n_stn_fc + 1 : 0) && (l.cin & 3) != 0) {
      l.ldw = (l.cin + 3) & ~3;
      l.Wpad = cv.take<float>((size_t)l.cout * l.ldw);
    }
    if (l.conv && !pl.training) l.Wpack = cv.take<float>(spg_conv_stack_packed_floats(l.cin, l.cout));
    if (l.conv && pl.training && l.cin % SPG_KC == 0) {      // layers the full-tile GEMM path can take (whole reduction chunks)
      l.Wb_f = cv.take<char>(spg_split_bytes(l.cout, l.cin));
      l.Wb_t = cv.take<char>(spg_split_bytes(l.cin, l.cout));
    }
  }
  if (pl.training) {
    size_t words = 0;
    for (const Layer& l : pl.L) if (l.bn) words += 2 * spg_fold_slot_words(l.cout);
    // + per segment the slots of the input's Gram matrix (the first two convolutions as one pass, spg_narrow.hip): inside the
    // same region, so they are cleared with the layers' slots
    const size_t gw_stn = pl.has_stn ? spg_gram_slot_words(c.nfeat_stn) : 0, gw_main = spg_gram_slot_words(c.nfeat);
    words += gw_stn + gw_main;
    pl.slots_all = cv.take<unsigned long long>(words); pl.slots_words = words;
    size_t off = 0;
    for (Layer& l : pl.L)
      if (l.bn) {
        l.slots = pl.slots_all ? pl.slots_all + off : nullptr; off += spg_fold_slot_words(l.cout);
        l.slots_bwd = pl.slots_all ? pl.slots_all + off : nullptr; off += spg_fold_slot_words(l.cout);
      }
    if (pl.has_stn) { pl.stn.gram = pl.slots_all ? pl.slots_all + off : nullptr; off += gw_stn; }
    pl.main.gram = pl.slots_all ? pl.slots_all + off : nullptr; off += gw_main;
  }
  const int Bc = pl.Bc;
  if (pl.S > 1) {
    pl.seg_clouds = cv.take<float>((size_t)pl.M * c.nfeat);
    pl.seg_T = cv.take<float>((size_t)Bc * 4);
  }
  auto carve_segment = [&](Segment& sg, float* final_out) {
    for (size_t k = 0; k < sg.convs.size(); ++k) {
      Layer& l = pl.L[sg.convs[k]];
      const bool last = k + 1 == sg.convs.size();
      l.ldy = l.cout;
      // the pooled layer's dense output is only needed by the backward pass
      l.y = (!last || pl.training) ? cv.take<float>((size_t)pl.M * l.cout) : nullptr;
    }
    const Layer& lc = pl.L[sg.convs.back()];
    sg.ldpool = (lc.cout + sg.nextra + 3) & ~3;      // padded: rows readable as aligned float4
    sg.pooled = cv.take<float>((size_t)B * sg.ldpool);
    sg.aidx = cv.take<int>((size_t)B * sg.ldpool);
    sg.spool = sg.pooled; sg.sidx = sg.aidx; sg.ldseg = sg.ldpool;
    if (pl.S > 1) {
      sg.ldseg = (lc.cout + 3) & ~3;
      sg.spool = cv.take<float>((size_t)Bc * sg.ldseg);
      sg.sidx = cv.take<int>((size_t)Bc * sg.ldseg);
    }
    for (size_t k = 0; k < sg.fcs.size(); ++k) {
      Layer& l = pl.L[sg.fcs[k]];
      const bool last = k + 1 == sg.fcs.size();
      l.ldy = l.cout;
      l.y = (last && final_out) ? final_out : cv.take<float>((size_t)B * l.cout);
    }
  };
  if (pl.has_stn) carve_segment(pl.stn, nullptr);
  carve_segment(pl.main, emb);
  pl.stat = cv.take<float>((size_t)Bc * 4 * 2 * cmax);      // up to 4 per-wave partials per tile
  pl.stat_cnt = cv.take<float>((size_t)Bc * 4 + 64);
  pl.fin = cv.take<double>(spg_bn_finalize_scratch_doubles(cmax));
  pl.pmax = cv.take<float>((size_t)Bc * 4 * cmax); pl.pmin = cv.take<float>((size_t)Bc * 4 * cmax);
  pl.imax = cv.take<int>((size_t)Bc * 4 * cmax); pl.imin = cv.take<int>((size_t)Bc * 4 * cmax);
  pl.bytes = cv.off + 256;
  return 0;
}

SpgOperand op_cloud(const Plan& pl, const float* clouds, const float* stnT) {
  SpgOperand o; memset(&o, 0, sizeof(o));
  o.mode = SPG_PRO_CLOUD; o.X = clouds; o.Ctot = pl.cfg.nfeat; o.P = pl.Pc; o.stnT = stnT;
  return o;
}

// the operand through which layer `k` of the segment reads its input in the forward pass
SpgOperand input_operand(const Plan& pl, const Segment& sg, bool is_fc, size_t k, const float* clouds, const float* stnT) {
  if (!is_fc) {
    if (k == 0) return op_cloud(pl, clouds, stnT);
    const Layer& p = pl.L[sg.convs[k - 1]];
    return spg_op_affine(p, p.y, p.ldy);
  }
  if (k == 0) {
    const Layer& p = pl.L[sg.convs.back()];
    return spg_op_affine(p, sg.pooled, sg.ldpool);
  }
  const Layer& p = pl.L[sg.fcs[k - 1]];
  return spg_op_affine(p, p.y, p.ldy);
}

// the BatchNorm side of one pass (spg_dense.h)
SpgDenseBn bn_of(const Plan& pl, int update_times, float* stat, double* fin, float* consts) {
  SpgDenseBn bn;
  bn.training = pl.training; bn.fold = pl.fold; bn.update_times = update_times;
  bn.momentum = pl.cfg.bn_momentum; bn.eps = pl.cfg.bn_eps;
  bn.stat = stat; bn.stat_cnt = pl.stat_cnt; bn.fin = fin; bn.consts = consts;
  return bn;
}

// inference: the whole convolution stack + max-pool of a segment in one kernel (spg_convstack.hip), when its shape allows
bool fused_eval_convs(Plan& pl, Segment& sg, const float* clouds, const float* stnT, SpgConvStackParams& cp) {
  if (pl.training || sg.convs.size() > SPG_CONVSTACK_MAX_LAYERS) return false;
  memset(&cp, 0, sizeof(cp));
  cp.clouds = clouds; cp.stnT = stnT; cp.B = pl.Bc; cp.P = pl.Pc; cp.Ctot = pl.cfg.nfeat; cp.nlayers = (int)sg.convs.size();
  for (size_t k = 0; k < sg.convs.size(); ++k) {
    const Layer& l = pl.L[sg.convs[k]];
    if (!l.bn) return false;
    cp.cin[k] = l.cin; cp.cout[k] = l.cout; cp.W[k] = l.W; cp.bias[k] = l.b; cp.s[k] = l.s; cp.t[k] = l.t;
    cp.Wp[k] = reinterpret_cast<f32x4*>(l.Wpack);
  }
  cp.pmax = pl.pmax; cp.pmin = pl.pmin;
  return spg_conv_stack_eval_supported(cp);
}

int forward_segment(Plan& pl, Segment& sg, const float* clouds, const float* stnT, int update_times, hipStream_t st) {
  SpgConvStackParams cp;
  const bool fused = fused_eval_convs(pl, sg, clouds, stnT, cp);
  if (fused) {
    const Layer& ll = pl.L[sg.convs.back()];
    SPG_TRY(spg_launch_conv_stack_eval(cp, st));
    if (pl.S > 1) {      // per pseudo-superpoint first, then over the segments of a superpoint (no winners: nothing reads them)
      SPG_TRY(spg_launch_pool_select_parts(pl.pmax, pl.pmin, nullptr, nullptr, ll.s, pl.Bc, ll.cout, 4, nullptr, 0, sg.spool, sg.ldseg,
                                           nullptr, st));
      SPG_TRY(spg_launch_pool_merge(sg.spool, nullptr, sg.ldseg, ll.s, pl.B, pl.S, pl.Pc, ll.cout, sg.extra, sg.nextra, sg.pooled,
                                    nullptr, sg.ldpool, st));
    } else {
      SPG_TRY(spg_launch_pool_select_parts(pl.pmax, pl.pmin, nullptr, nullptr, ll.s, pl.B, ll.cout, 4, sg.extra, sg.nextra,
                                           sg.pooled, sg.ldpool, nullptr, st));
    }
  }
  size_t kfirst = 0;
  if (pl.training && sg.gram != nullptr) gram_record(sg.gram, false);      // (set below when this forward fills the Gram slots)
  // train mode: the first two convolutions (cloud -> 64 -> 64) as ONE pass over the points -- the first layer's batch statistics
  // from the Gram matrix of the input, its raw output written once and never read back (spg_narrow.hip)
  if (!fused && pl.training && pl.fold && sg.gram != nullptr && sg.convs.size() > 2) {
    Layer& l0 = pl.L[sg.convs[0]];
    Layer& l1 = pl.L[sg.convs[1]];
    if (l0.bn && l1.bn && spg_narrow_pair_supported(l0.cin, l0.cout, l1.cout, pl.Pc, pl.M)) {
      SpgGramParams gp; memset(&gp, 0, sizeof(gp));
      gp.clouds = clouds; gp.stnT = stnT; gp.B = pl.Bc; gp.P = pl.Pc; gp.Ctot = pl.cfg.nfeat; gp.nfeat = l0.cin; gp.gram = sg.gram;
      SPG_TRY(spg_launch_cloud_gram(gp, st));
      SPG_TRY(spg_slot_sync_after(sg.gram, spg_gram_slot_words(l0.cin), st, false));      // (slot-synchronised BatchNorm)
      SpgNarrowPairParams np; memset(&np, 0, sizeof(np));
      np.clouds = clouds; np.stnT = stnT; np.P = pl.Pc; np.Ctot = pl.cfg.nfeat; np.nfeat = l0.cin; np.nblk = (int)(pl.M / 32);
      np.count = (double)pl.M;
      np.W1 = l0.W; np.b1 = l0.b; np.y1 = l0.y; np.gram = sg.gram; np.gamma1 = l0.gamma; np.beta1 = l0.beta; np.rm1 = l0.rm; np.rv1 = l0.rv;
      np.mean1 = l0.mean; np.rstd1 = l0.rstd; np.s1 = l0.s; np.t1 = l0.t;
      np.update_times = update_times; np.momentum = pl.cfg.bn_momentum; np.eps = pl.cfg.bn_eps;
      np.W2 = l1.W; np.b2 = l1.b; np.y2 = l1.y; np.slots2 = l1.slots;
      SPG_TRY(spg_launch_narrow_pair_fwd(np, st));
      SPG_TRY(spg_slot_sync_after(l1.slots, spg_fold_slot_words(l1.cout), st, false));
      gram_record(sg.gram, true);
      kfirst = 2;
    }
  }
  for (size_t k = kfirst; !fused && k < sg.convs.size(); ++k) {
    Layer& l = pl.L[sg.convs[k]];
    const bool last = k + 1 == sg.convs.size();
    SpgGemmParams g; memset(&g, 0, sizeof(g));
    g.a = input_operand(pl, sg, false, k, clouds, stnT);
    if (k > 0 && pl.fold) g.fold = spg_fold_of(pl.L[sg.convs[k - 1]], pl.M, update_times, pl.cfg.bn_momentum, pl.cfg.bn_eps);
    g.W = l.W; g.ldw = l.cin; g.bias = l.b; g.M = (int)pl.M; g.N = l.cout; g.K = l.cin;
    g.rows_per_tile = pl.Pc; g.epi = SPG_EPI_FWD; g.Y = l.y; g.ldy = l.ldy;
    if (l.Wb_f != nullptr) { g.Wb = l.Wb_f; g.ldwb = spg_split_ld(l.cin); g.wb_part_bytes = (long)l.cout * g.ldwb * 2; }
    if (last && !pl.training) g.Y = nullptr;     // inference: only the pooled values of the last conv are consumed
    g.stat = pl.training ? pl.stat : nullptr; g.stat_cnt = pl.stat_cnt;
    if (pl.fold) { g.stat = nullptr; g.stat_slots = l.slots; }
    int nparts = 0;
    if (last) {      // max-pool fused into the epilogue: the sign of the BatchNorm scale is the sign of gamma
      g.pool_out = sg.spool; g.pool_idx = sg.sidx; g.pool_ld = sg.ldseg; g.pool_sign = l.gamma;
      if (pl.S == 1) { g.pool_extra = sg.extra; g.pool_nextra = sg.nextra; }      // (else appended by the merge)
    }
    SPG_TRY(spg_launch_gemm(g, st, &nparts));
    if (last && pl.S > 1)      // the segments' extrema -> the superpoint's, by the epilogue's rule (the sign of gamma)
      SPG_TRY(spg_launch_pool_merge(sg.spool, sg.sidx, sg.ldseg, l.gamma, pl.B, pl.S, pl.Pc, l.cout, sg.extra, sg.nextra, sg.pooled,
                                    sg.aidx, sg.ldpool, st));
    if (pl.training && !pl.fold)      // (eval mode: one spg_launch_bn_eval_batch at the start of the forward)
      SPG_TRY(spg_launch_bn_finalize(pl.stat, pl.stat_cnt, nparts, pl.M, l.cout, l.gamma, l.beta, l.rm, l.rv,
                                     pl.cfg.bn_momentum, pl.cfg.bn_eps, update_times, l.mean, l.rstd, l.s, l.t, pl.fin, st));
  }
  // every FC layer is a few-row launch: issued through a group scope (a group of one, or of two with the weight padding below),
  // so that a rider chain of the caller -- the filter network's forward -- can leave with it (spg_gemm.h)
  SpgGroupScope grp(st);
  for (size_t k = 0; k < sg.fcs.size(); ++k) {
    Layer& l = pl.L[sg.fcs[k]];
    // zero-padded weight copies (input widths that are no multiples of 4: 256 pooled channels + the diameter): they depend on
    // the weights only -- all of them leave with the FIRST few-row launch of the forward that does not need one itself
    if (!pl.pads_done) {
      bool mine = false;
      for (int idx : sg.fcs) mine = mine || pl.L[idx].Wpad != nullptr;
      if (mine && k == 0) {      // this segment's own layers need them: a launch of their own, in front
        for (Layer& q : pl.L) if (q.Wpad) SPG_TRY(spg_launch_pad_rows(q.W, q.cin, q.Wpad, q.ldw, q.cout, q.cin, st));
        SPG_TRY(grp.flush());
      } else if (!mine) {
        for (Layer& q : pl.L) if (q.Wpad) SPG_TRY(spg_launch_pad_rows(q.W, q.cin, q.Wpad, q.ldw, q.cout, q.cin, st));
      }
      pl.pads_done = true;
    }
    // the producer's statistics: the last convolution (over all points) for the first fc layer, else the previous fc layer
    const Layer& prod = k == 0 ? pl.L[sg.convs.back()] : pl.L[sg.fcs[k - 1]];
    SPG_TRY(spg_dense_forward(l, &prod, input_operand(pl, sg, true, k, clouds, stnT), pl.B, k == 0 ? pl.M : (long)pl.B,
                              bn_of(pl, update_times, pl.stat, pl.fin, nullptr), &grp, st));
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
struct BwdScratch {
  float *dzA = nullptr, *dzB = nullptr;     // [M, cmax_conv] ping-pong for the dense conv gradients
  float *fzA = nullptr, *fzB = nullptr;     // [B, cmax_fc]
  float* consts = nullptr;                  // [4][cmax]
  double* fin = nullptr;                    // scratch of the sliced finalize
  float* work = nullptr;                    // reduction arena: split partials of all weight / bias gradients
  size_t work_floats = 0;
  float* stat = nullptr;                    // [ntile][2][cmax]
  float* dxy = nullptr;                     // [M, 2]
  float* dT = nullptr;                      // [B, 4]
  // npts > 128 (spg_segments.h): the pooled gradient and the winners in the segments' view [Bc, ldseg]; per-segment partials [Bc, 4] of dT
  float* gseg = nullptr;
  int* lidx = nullptr;
  float* dTseg = nullptr;
  float* grad_global = nullptr;             // optional output [B, nextra]: gradient wrt the concatenated global features
  size_t bytes = 0;
};

void carve_bwd(const Plan& pl, void* ws, BwdScratch& s) {
  SpgCarver cv(ws);
  int cconv = 4, cfc = 4, cmax = 4;
  size_t wmax = 16, workmax = 16;
  for (const Layer& l : pl.L) {
    if (l.conv) { cconv = l.cin > cconv ? l.cin : cconv; }
    else { cfc = l.cin + 4 > cfc ? l.cin + 4 : cfc; }
    cmax = l.cout > cmax ? l.cout : cmax; cmax = l.cin > cmax ? l.cin : cmax;
    wmax = (size_t)l.cin * l.cout > wmax ? (size_t)l.cin * l.cout : wmax;
    // every layer gets its own slice of the reduction arena (partials stay alive until the single batched reduce)
    workmax += spg_queue_layer_floats(l.conv ? pl.M : pl.B, l.cout, l.cin);
    // (the one-pass backward of a segment's first convolution writes one partial per wave, spg_narrow.h)
    if (l.conv && l.cin <= SPG_GRAM_MAXF) workmax += ((size_t)spg_first_conv_bwd_partials(pl.Bc) * l.cout * l.cin + 63) & ~(size_t)63;
  }
  s.dzA = cv.take<float>((size_t)pl.M * cconv); s.dzB = cv.take<float>((size_t)pl.M * cconv);
  s.fzA = cv.take<float>((size_t)pl.B * cfc); s.fzB = cv.take<float>((size_t)pl.B * cfc);
  s.consts = cv.take<float>((size_t)4 * cmax);
  s.fin = cv.take<double>(spg_bn_finalize_scratch_doubles(cmax));
  s.work = cv.take<float>(workmax); s.work_floats = workmax;
  s.stat = cv.take<float>((size_t)pl.Bc * 4 * 2 * cmax);
  s.dxy = cv.take<float>((size_t)pl.M * 2);
  s.dT = cv.take<float>((size_t)pl.B * 4);
  if (pl.S > 1) {
    const size_t ldmax = pl.has_stn && pl.stn.ldseg > pl.main.ldseg ? pl.stn.ldseg : pl.main.ldseg;      // (the stacks run one after the other)
    s.gseg = cv.take<float>((size_t)pl.Bc * ldmax); s.lidx = cv.take<int>((size_t)pl.Bc * ldmax);
    s.dTseg = cv.take<float>((size_t)pl.Bc * 4);
  }
  s.bytes = cv.off + 256;
}

// Backward of one segment.  `cur` is the gradient wrt the raw output of the segment's last fc layer
// (IDENT operand).  If want_dxy, the gradient wrt the first two input channels of conv 0 is left in s.dxy.
// dT_out / dT_done: with want_dxy, the one-pass backward of the first convolution (spg_narrow.h) writes the gradient of the 2 x 2
// transforms [B, 4] itself and sets *dT_done; otherwise s.dxy holds the gradient wrt the transformed xy for spg_launch_stn_dT
int backward_segment(Plan& pl, Segment& sg, BwdScratch& s, SpgReduceQueue& rq, SpgOperand cur, const float* clouds,
                     const float* stnT, bool want_dxy, hipStream_t st, bool ride_reduce = false,
                     float* dT_out = nullptr, bool* dT_done = nullptr) {
  const int B = pl.B;
  SpgBnFoldBwd pending; memset(&pending, 0, sizeof(pending));     // set by a data-gradient launch, consumed by the next weight gradient
  // ---- fc head ----
  // A layer's weight gradient and its data gradient depend on the same inputs and not on each other: both few-row launches
  // leave as ONE grouped launch (spg_gemm.h) -- three launches per head instead of six (spg_dense_backward).
  float* fz[2] = {s.fzA, s.fzB};
  int flip = 0;
  const float* pooled_grad = nullptr;
  {
  SpgGroupScope grp(st);
  // the split partials the launches so far have queued (the other segment's weight gradients: ~100 MB, 2/3 of the step's final
  // reduction) are summed as jobs of this segment's grouped launches -- a slice of ~35 MB each -- in the shadow of its
  // latency-bound FC layers
  for (int k = (int)sg.fcs.size() - 1; k >= 0; --k) {
    if (ride_reduce) SPG_TRY(spg_reduce_ride(rq, st));      // (a slice per group; before this layer queues its own partials)
    Layer& l = pl.L[sg.fcs[k]];
    // data gradient -> producer of this layer's input; the first fc layer reads the pooled rows of the last convolution, whose
    // statistics run over all points
    const bool first = k == 0;
    Layer& prod = first ? pl.L[sg.convs.back()] : pl.L[sg.fcs[k - 1]];
    float* out = fz[flip]; flip ^= 1;
    SpgDenseDgrad d;
    d.prod = &prod; d.out = out; d.ldout = first ? sg.ldpool : l.cin;
    d.Yp = first ? sg.pooled : prod.y; d.ldyp = first ? sg.ldpool : prod.ldy;
    d.count = d.stat_rows = first ? pl.M : (long)B;
    d.folds = grp.active();      // (separate launches: the weight gradient runs first and finishes the constants)
    SPG_TRY(spg_dense_backward(rq, l, cur, input_operand(pl, sg, true, k, clouds, stnT), B, d, bn_of(pl, 1, s.stat, s.fin, s.consts),
                               pending, &grp, st));      // flushed: {weight gradient, bias column sums, data gradient} of this layer
    const int C = prod.cout;
    if (first && s.grad_global != nullptr && sg.nextra > 0)     // columns >= C pass through: gradient wrt the global features
      SPG_TRY(spg_launch_copy2d(out + C, sg.ldpool, s.grad_global, sg.nextra, B, sg.nextra, st));
    if (!first) {
      cur = spg_op_bnbwd(out, prod.y, prod.ldy, s.consts, C);
    } else {
      memset(&cur, 0, sizeof(cur));
      cur.mode = SPG_PRO_POOLBWD; cur.X = out; cur.ldg = (int)sg.ldpool; cur.aidx = sg.aidx; cur.P = pl.Pc;
      if (pl.S > 1) { cur.X = s.gseg; cur.ldg = (int)sg.ldseg; cur.aidx = s.lidx; pooled_grad = out; }      // (filled behind the head, below)
      cur.X2 = prod.y; cur.ld = prod.ldy;
      cur.c0 = s.consts; cur.c1 = s.consts + C; cur.c2 = s.consts + 2 * C; cur.c3 = s.consts + 3 * C;
    }
  }
  }      // (the group scope ends with the head: the convolutions' launches are ordered, never grouped)
  if (pl.S > 1)      // the head's pooled gradient [B, ldpool] and the merged winners -> what the POOLBWD operand reads per pseudo-superpoint
    SPG_TRY(spg_launch_pool_expand(pooled_grad, sg.aidx, sg.ldpool, B, pl.S, pl.Pc, pl.L[sg.convs.back()].cout, s.gseg, s.lidx, sg.ldseg, st));
  // ---- conv stack ----
  float* dz[2] = {s.dzA, s.dzB};
  flip = 0;
  for (int k = (int)sg.convs.size() - 1; k >= 0; --k) {
    Layer& l = pl.L[sg.convs[k]];
    if (k > 0 && pl.fold) {      // (pending: this layer's sums, or none when a finalize launch already made the constants)
      // 64-input-channel layers: data gradient + weight gradient from ONE pass over dz (spg_gemm.h: spg_queue_bwdpair)
      Layer& prod = pl.L[sg.convs[k - 1]];
      float* out = dz[flip];
      SpgGemmParams g; memset(&g, 0, sizeof(g));
      g.a = cur; g.W = l.W; g.ldw = l.cin; g.w_red = 1;
      g.M = (int)pl.M; g.N = l.cin; g.K = l.cout; g.rows_per_tile = pl.Pc;
      g.epi = SPG_EPI_BWD; g.Y = out; g.ldy = l.cin; g.Yp = prod.y; g.ldyp = prod.ldy;
      g.ms = prod.s; g.mt = prod.t; g.mask_relu = 1; g.n_mask = prod.cout;
      g.mmean = prod.mean; g.mrstd = prod.rstd; g.stat_slots = prod.slots_bwd; g.fold_bwd = pending;
      const SpgOperand xin = input_operand(pl, sg, false, k, clouds, stnT);
      if (spg_bwdpair_supported(g, xin)) {
        SPG_TRY(spg_queue_bwdpair(rq, g, xin, l.dW, st));
        if (l.db) SPG_TRY(spg_zero_bytes_async(l.db, sizeof(float) * l.cout, st));
        flip ^= 1;
        pending = spg_fold_bwd_of(prod, pl.M, s.consts);      // (the launch consumed this layer's; these are the producer's)
        cur = spg_op_bnbwd(out, prod.y, prod.ldy, s.consts, prod.cout);
        continue;
      }
    }
    // The FIRST convolution behind a forward that left the Gram matrix of the input in the slots (spg_narrow.hip): weight gradient
    // and -- main segment behind an STN -- the gradient of the 2 x 2 transforms from ONE pass over the incoming gradient and the
    // cloud; the layer's raw output is not read (it is linear in the cloud: its part collapses onto the Gram matrix)
    if (k == 0 && pl.fold && sg.gram != nullptr && gram_recorded(sg.gram) && sg.convs.size() > 2 && pending.slots != nullptr && cur.mode == SPG_PRO_BNBWD &&
        cur.ld == l.cout && cur.c0 == s.consts && (!want_dxy || dT_out != nullptr) &&
        spg_narrow_pair_supported(l.cin, l.cout, pl.L[sg.convs[1]].cout, pl.Pc, pl.M) && spg_first_conv_bwd_supported(l.cin, l.cout, pl.Pc, pl.M)) {
      SpgFirstConvBwdParams fp; memset(&fp, 0, sizeof(fp));
      fp.clouds = clouds; fp.stnT = stnT; fp.B = pl.Bc; fp.P = pl.Pc; fp.Ctot = pl.cfg.nfeat; fp.nfeat = l.cin;
      fp.g = cur.X; fp.W1 = l.W; fp.gram = sg.gram; fp.fold = pending; memset(&pending, 0, sizeof(pending));
      fp.dT = want_dxy ? (pl.S > 1 ? s.dTseg : dT_out) : nullptr;
      SPG_TRY(spg_queue_partials(rq, spg_first_conv_bwd_partials(pl.Bc), l.cout * l.cin, l.dW, &fp.partial, st));
      SPG_TRY(spg_launch_first_conv_bwd(fp, st));
      if (want_dxy && pl.S > 1) SPG_TRY(spg_launch_segment_dT_sum(s.dTseg, B, pl.S, dT_out, st));      // (segments in fixed order)
      if (l.db) SPG_TRY(spg_zero_bytes_async(l.db, sizeof(float) * l.cout, st));
      if (want_dxy && dT_done != nullptr) *dT_done = true;
      continue;
    }
    SpgWgradParams w; memset(&w, 0, sizeof(w));
    w.a = cur; w.b = input_operand(pl, sg, false, k, clouds, stnT); w.M = (int)pl.M; w.N = l.cout; w.K = l.cin;
    w.fold = pending; memset(&pending, 0, sizeof(pending));
    w.allow_lowp = 1;      // the opt-in precision modes act on the PointNet convolutions only
    SPG_TRY(spg_queue_wgrad(rq, w, l.dW, st));
    if (l.db) SPG_TRY(spg_zero_bytes_async(l.db, sizeof(float) * l.cout, st));
    if (k > 0) {
      Layer& prod = pl.L[sg.convs[k - 1]];
      float* out = dz[flip]; flip ^= 1;
      SpgGemmParams g; memset(&g, 0, sizeof(g));
      g.a = cur; g.W = l.W; g.ldw = l.cin; g.w_red = 1;
      g.M = (int)pl.M; g.N = l.cin; g.K = l.cout; g.rows_per_tile = pl.Pc;
      if (l.Wb_t != nullptr) { g.Wb = l.Wb_t; g.ldwb = spg_split_ld(l.cout); g.wb_part_bytes = (long)l.cin * g.ldwb * 2; }
      g.epi = SPG_EPI_BWD; g.Y = out; g.ldy = l.cin; g.Yp = prod.y; g.ldyp = prod.ldy;
      g.ms = prod.s; g.mt = prod.t; g.mask_relu = 1; g.n_mask = prod.cout;
      g.mmean = prod.mean; g.mrstd = prod.rstd; g.stat = s.stat;
      const bool foldk = pl.fold && !spg_gemm_bwd_stats_want_partials(g);
      if (foldk) { g.stat = nullptr; g.stat_slots = prod.slots_bwd; }
      int nparts = 0;
      SPG_TRY(spg_launch_gemm(g, st, &nparts));
      if (foldk) pending = spg_fold_bwd_of(prod, pl.M, s.consts);
      else
      SPG_TRY(spg_launch_bn_bwd_finalize(s.stat, nparts, l.cin, pl.M, prod.cout, prod.s, prod.mean, prod.rstd, s.consts,
                                         prod.dgamma, prod.dbeta, s.fin, st));
      cur = spg_op_bnbwd(out, prod.y, prod.ldy, s.consts, prod.cout);
    } else if (want_dxy) {
      // gradient wrt the transformed xy only (learning/pointnet.py:123-124): 2 output columns
      SpgGemmParams g; memset(&g, 0, sizeof(g));
      g.a = cur; g.W = l.Wpad ? l.Wpad : l.W; g.ldw = l.Wpad ? l.ldw : l.cin; g.w_red = 1;
      g.M = (int)pl.M; g.N = 2; g.K = l.cout; g.rows_per_tile = pl.Pc;
      g.epi = SPG_EPI_BWD; g.Y = s.dxy; g.ldy = 2;
      SPG_TRY(spg_launch_gemm(g, st));
    }
  }
  return 0;
}

}  // namespace

extern "C" int spg_pointnet_num_layers(const spg_pointnet_cfg* cfg) { return cfg ? num_layers(*cfg) : -1; }

extern "C" size_t spg_pointnet_workspace_bytes(const spg_pointnet_cfg* cfg, int B, int training) {
  Plan pl;
  if (make_plan(cfg, B, training, nullptr, nullptr, nullptr, pl) != 0) return 0;
  return pl.bytes;
}

extern "C" int spg_pointnet_forward(const spg_pointnet_cfg* cfg, int B, const float* clouds, const float* clouds_global,
                                    const void* const* params, float* emb, void* workspace, int training,
                                    int bn_update_times, void* stream) {
  return spg_pointnet_forward_ext(cfg, B, clouds, clouds_global, nullptr, params, emb, workspace, training, bn_update_times, stream);
}

// spg_train_step (spg_step.hip), per thread: `clean` -- a train-mode forward does NOT clear the statistics slots (the caller
// vouches that the previous step on the same workspace left them zero); `clear_at_end` -- the backward clears them as a job of
// its final batched reduction (a reduction over ZERO partials writes zeros): the last launch of the step, behind every producer
// and consumer of the slots
static thread_local bool g_slots_clean = false, g_slots_clear_at_end = false;
void spg_pointnet_set_step_flags(bool clean, bool clear_at_end) { g_slots_clean = clean; g_slots_clear_at_end = clear_at_end; }

extern "C" int spg_pointnet_forward_ext(const spg_pointnet_cfg* cfg, int B, const float* clouds, const float* clouds_global,
                                        const float* ext_transform, const void* const* params, float* emb, void* workspace,
                                        int training, int bn_update_times, void* stream) {
  SPG_CHECK_ARG(clouds && params && emb && workspace, "null pointer");
  SPG_CHECK_ARG(ext_transform == nullptr || cfg->nfeat_stn == 0, "an external transform replaces the inner STN (nfeat_stn must be 0)");
  hipStream_t st = (hipStream_t)stream;
  Plan pl;
  SPG_TRY(make_plan(cfg, B, training, workspace, params, emb, pl));
  SPG_CHECK_ARG(pl.cfg.nfeat_global == 0 || clouds_global != nullptr, "clouds_global is required");
  pl.main.extra = clouds_global;
  if (!pl.training) {        // eval mode: the BatchNorm constants of every layer in one launch
    SpgBnEvalBatch eb;
    for (Layer& l : pl.L)
      if (l.bn) {
        SPG_CHECK_ARG(eb.njobs < SPG_BN_EVAL_MAX_JOBS, "too many BatchNorm layers");
        eb.jobs[eb.njobs++] = SpgBnEvalJob{l.cout, l.gamma, l.beta, l.rm, l.rv, l.s, l.t};
      }
    SPG_TRY(spg_launch_bn_eval_batch(eb, pl.cfg.bn_eps, st));
  }
  if (pl.training && spg_gemm_precision() != 0) {      // opt-in bf16 / split-bf16 MFMA: bf16 copies of the conv weights, one launch
    SpgSplitBatch sb;
    for (Layer& l : pl.L)
      if (l.Wb_f != nullptr) {
        SPG_CHECK_ARG(sb.njobs < SPG_SPLIT_MAX_JOBS, "too many layers");
        sb.jobs[sb.njobs++] = SpgSplitJob{l.W, l.cin, l.cout, l.cin, l.Wb_f, l.Wb_t};
      }
    SPG_TRY(spg_launch_split_weights(sb, st));
  }
  // train mode: the BatchNorm statistics travel as slots from each producer GEMM to its consumer; every tile
  // contributes at most 4 wave partials per channel: within the slots' capacity up to ~500 k superpoints
  pl.fold = pl.training && spg_bn_fold_allowed(4L * pl.Bc);
  SPG_TRY(spg_bn_slot_sync_check(pl.training, pl.fold, "slot-synchronised BatchNorm needs the statistics slots (spg_tune key 10 off, batch within the slots' capacity)"));
  if (pl.training && !g_slots_clean) {      // always in train mode: the backward decides about its own slots independently (they are cleared here too)
    hipError_t me = hipMemsetAsync(pl.slots_all, 0, pl.slots_words * sizeof(unsigned long long), st);
    if (me != hipSuccess) { spg_set_error("hipMemsetAsync: %s", hipGetErrorString(me)); return (int)me; }
  }
  const float* stnT = ext_transform;      // [B, 4] = T - I of an externally evaluated STN (LocalCloudEmbedder), or null
  if (pl.S > 1) {      // npts > 128: the convolutions read the clouds per segment (spg_segments.h); the backward reads the same copy
    SPG_TRY(spg_launch_segment_clouds(clouds, B, pl.cfg.nfeat, pl.P, pl.Pc, pl.seg_clouds, st));
    clouds = pl.seg_clouds;
  }
  if (pl.has_stn) {
    SPG_TRY(forward_segment(pl, pl.stn, clouds, nullptr, bn_update_times, st));
    stnT = pl.L[pl.stn.fcs.back()].y;
  }
  if (pl.S > 1 && stnT != nullptr) {      // a superpoint's transform for each of its segments
    SPG_TRY(spg_launch_segment_transforms(stnT, B, pl.S, pl.seg_T, st));
    stnT = pl.seg_T;
  }
  SPG_TRY(forward_segment(pl, pl.main, clouds, stnT, bn_update_times, st));
  return 0;
}

// debug / test helper: byte offset inside the forward workspace of a layer's buffers
//   what: 0 raw output y, 1 BN scale s, 2 BN shift t, 3 batch mean, 4 batch rstd;
//   layer == -1 / -2: STN / main segment; what 0: pooled [B, ldpool] (selected raw max/min + globals), what 1: aidx [B, ldpool]
//   (int32: the point that holds the pooled value), what 2: ldpool itself (not an offset).
extern "C" long spg_pointnet_debug_offset(const spg_pointnet_cfg* cfg, int B, int training, int layer, int what) {
  Plan pl;
  char* fake = (char*)(uintptr_t)4096;
  if (make_plan(cfg, B, training, fake, nullptr, (float*)(uintptr_t)8, pl) != 0) return -1;
  const void* p = nullptr;
  if (layer == -1 || layer == -2) {
    const Segment& sg = layer == -1 ? pl.stn : pl.main;
    if (layer == -1 && !pl.has_stn) return -1;
    if (what == 2) return sg.ldpool;
    p = what == 1 ? (const void*)sg.aidx : (const void*)sg.pooled;
  }
  else if (layer >= 0 && layer < (int)pl.L.size()) {
    const Layer& l = pl.L[layer];
    p = what == 0 ? (const void*)l.y : what == 1 ? l.s : what == 2 ? l.t : what == 3 ? l.mean : l.rstd;
    if (what == 0 && l.y == (float*)(uintptr_t)8) return -1;
  }
  if (p == nullptr) return -1;
  return (long)((const char*)p - fake);
}

extern "C" size_t spg_pointnet_bwd_workspace_bytes(const spg_pointnet_cfg* cfg, int B) {
  Plan pl;
  if (make_plan(cfg, B, 1, nullptr, nullptr, nullptr, pl) != 0) return 0;
  BwdScratch s;
  carve_bwd(pl, nullptr, s);
  return s.bytes;
}

extern "C" int spg_pointnet_backward(const spg_pointnet_cfg* cfg, int B, const float* clouds, const float* clouds_global,
                                     const void* const* params, const float* grad_emb, void* const* grads,
                                     void* workspace, void* bwd_workspace, void* stream) {
  return spg_pointnet_backward_ext(cfg, B, clouds, clouds_global, nullptr, params, grad_emb, grads, nullptr, nullptr, workspace,
                                   bwd_workspace, stream);
}

extern "C" int spg_pointnet_backward_ext(const spg_pointnet_cfg* cfg, int B, const float* clouds, const float* clouds_global,
                                         const float* ext_transform, const void* const* params, const float* grad_emb,
                                         void* const* grads, float* grad_transform, float* grad_global, void* workspace,
                                         void* bwd_workspace, void* stream) {
  SPG_CHECK_ARG(clouds && params && grad_emb && grads && workspace && bwd_workspace, "null pointer");
  SPG_CHECK_ARG((ext_transform == nullptr && grad_transform == nullptr) || cfg->nfeat_stn == 0, "external transform with an inner STN");
  SPG_CHECK_ARG(grad_transform == nullptr || ext_transform != nullptr, "grad_transform needs the external transform");
  hipStream_t st = (hipStream_t)stream;
  Plan pl;
  // the forward wrote the last fc output to `emb`; it is not needed by the backward, so pass a dummy
  SPG_TRY(make_plan(cfg, B, 1, workspace, params, (float*)grad_emb /*unused as y*/, pl));
  pl.main.extra = clouds_global;
  pl.fold = spg_bn_fold_allowed(4L * pl.Bc);
  for (size_t i = 0; i < pl.L.size(); ++i) spg_dense_bind_grads(pl.L[i], grads + 6 * i);
  BwdScratch s;
  carve_bwd(pl, bwd_workspace, s);
  const float* stnT = pl.has_stn ? pl.L[pl.stn.fcs.back()].y : ext_transform;
  const float* clouds_pts = clouds;      // [B, nfeat, P]: spg_launch_stn_dT walks the true P points of a superpoint (rows b * P + p of dxy)
  if (pl.S > 1) {      // the forward's copies in the segments' view
    clouds = pl.seg_clouds;
    if (stnT != nullptr) stnT = pl.seg_T;
  }
  const int cout = pl.L[pl.main.fcs.back()].cout;
  SpgReduceQueue rq;
  rq.arena = s.work; rq.arena_floats = s.work_floats;
  s.grad_global = grad_global;
  bool dT_done = false;
  float* dT_target = grad_transform != nullptr ? grad_transform : (pl.has_stn ? s.dT : nullptr);
  SPG_TRY(backward_segment(pl, pl.main, s, rq, spg_op_ident(grad_emb, cout), clouds, stnT, pl.has_stn || grad_transform != nullptr, st, false,
                           dT_target, &dT_done));
  if (grad_transform != nullptr && !dT_done)      // gradient wrt the external 2x2 transforms (learning/pointnet.py:196-198)
    SPG_TRY(spg_launch_stn_dT(clouds_pts, pl.cfg.nfeat, pl.P, B, s.dxy, 2, grad_transform, st));
  if (pl.has_stn) {
    if (!dT_done) SPG_TRY(spg_launch_stn_dT(clouds_pts, pl.cfg.nfeat, pl.P, B, s.dxy, 2, s.dT, st));
    SPG_TRY(backward_segment(pl, pl.stn, s, rq, spg_op_ident(s.dT, 4), clouds, nullptr, false, st, true));
  }
  if (g_slots_clear_at_end && pl.slots_all != nullptr && pl.slots_words > 0) {
    SPG_CHECK_ARG(2 * pl.slots_words < (size_t)INT_MAX, "statistics slots too large for one reduction job");
    SpgReduceJob j;
    j.partial = reinterpret_cast<const float*>(pl.slots_all); j.out = reinterpret_cast<float*>(pl.slots_all);
    j.nsplit = 0; j.n = (int)(2 * pl.slots_words);
    spg_reduce_defer(j);
  }
  return spg_flush_reduce(rq, st);      // ONE launch sums the split partials of all weight / bias gradients
}
