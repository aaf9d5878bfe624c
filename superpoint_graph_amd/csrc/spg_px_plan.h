// The launch plan of the one-launch GRU recurrences (spg_ecc.hip): which form a graph runs in, with how many workgroups.  Every
// workgroup of such a launch must be RESIDENT at the same time -- its waves spin on granules that other workgroups write -- so a
// grid one workgroup too large times out (the update is withheld) or hangs.  This is the one place that decides it.  Plain C++,
// nothing of HIP: tests/px_plan_host_test.cpp sweeps it on the host.
#pragma once

#define SPG_PX_WG_NODES 1024       // nodes per round with ONE 4-wave workgroup per CU (one wavefront per node, all co-resident)
#define SPG_PX_MAX_NODES 2048      // nodes per round with two workgroups per CU (fewer register-resident filters, gate rows from LDS)
#define SPG_PX_MAX_GROUPS 8        // rounds per launch: groups of whole connected components (scenes) of <= SPG_PX_MAX_NODES nodes
#define SPG_PX_MULTI_MAX_NODES 16000      // one group above SPG_PX_MAX_NODES: several nodes per wavefront, iteration-major (spg_ecc.hip)
#define SPG_PX_MAX_ITERS 16        // states h^0 .. h^R of a launch: R + 1 <= SPG_PX_MAX_ITERS
#define SPG_PX_MULTI_NPW 8         // nodes per wavefront of the iteration-major kernels, at most
#define SPG_PX_CU_MARGIN 4         // CUs the residency bound leaves to whatever else runs on the device

inline bool spg_px_is_multi(int n_groups, int max_group) { return n_groups == 1 && max_group > SPG_PX_MAX_NODES; }
struct SpgPxGroups {               // node ranges [ptr[g], ptr[g+1]) of the rounds; n = 1: the whole graph in one round
  int n;
  int ptr[SPG_PX_MAX_GROUPS + 1];
};
inline int spg_px_max_group(const SpgPxGroups& g) {      // largest round
  int m = 0;
  for (int k = 0; k < g.n; ++k) m = g.ptr[k + 1] - g.ptr[k] > m ? g.ptr[k + 1] - g.ptr[k] : m;
  return m;
}
// one round above SPG_PX_MAX_NODES nodes: the iteration-major kernels (no forward internals kept, no head)
inline bool spg_px_groups_multi(const SpgPxGroups& g) { return spg_px_is_multi(g.n, spg_px_max_group(g)); }

// Rounds for a batch whose connected components are unions of the node ranges part_ptr[0..n_parts] (scenes of a batch; n_parts
// = 0: unknown -- one round if the whole graph fits): consecutive parts are packed greedily into groups of at most
// SPG_PX_MAX_NODES nodes.  false when a part exceeds a round or too many rounds would be needed and the one-group form does
// not apply either.  key8 = spg_tune key 8 (2: the iteration-major form is off).
inline bool spg_px_plan_groups(int N, int n_parts, const int* part_ptr, int key8, SpgPxGroups* out) {
  const int cap = SPG_PX_MAX_NODES;
  out->n = 0;
  if (N <= 0) return false;
  if (N <= cap) { out->n = 1; out->ptr[0] = 0; out->ptr[1] = N; return true; }      // one round, whatever the components
  // components unknown, or one of them above a round: ONE group with several nodes per wavefront (the iteration-major kernels)
  auto big = [&]() -> bool {
    if (N > SPG_PX_MULTI_MAX_NODES || key8 == 2) return false;
    out->n = 1; out->ptr[0] = 0; out->ptr[1] = N;
    return true;
  };
  if (n_parts <= 0 || part_ptr == nullptr || part_ptr[0] != 0 || part_ptr[n_parts] != N) return big();
  int start = 0;
  out->ptr[0] = 0;
  for (int k = 0; k < n_parts; ++k) {
    const int a = part_ptr[k], b = part_ptr[k + 1];
    if (b < a) return false;
    if (b - a > cap) return big();
    if (b - start > cap) {                // part k opens a new group
      if (out->n + 1 >= SPG_PX_MAX_GROUPS) return big();
      out->ptr[++out->n] = a;
      start = a;
    }
  }
  out->ptr[++out->n] = N;
  return true;
}

// SPG_PX_DECLINED: the per-iteration launches.  ONE / TWO_PER_CU: one node per wavefront, that many 4-wave workgroups per CU.
// ITER_MAJOR: one round above SPG_PX_MAX_NODES nodes, several nodes per wavefront.
enum SpgPxForm { SPG_PX_DECLINED = 0, SPG_PX_ONE_PER_CU = 1, SPG_PX_TWO_PER_CU = 2, SPG_PX_ITER_MAJOR = 3 };
// what the service-workgroup rule of the backward reads of the head: the forward launch ran one; its parameter gradients may be
// formed in the launch (<= 16 classes, aligned, spg_tune key 6 off, the caller asks); its input width
struct SpgPxHeadFacts { bool present, wgrad; int nin; };
struct SpgPxPlan {                 // SPG_PX_DECLINED: every other field is 0
  SpgPxForm form;
  int wpc, node_wgs, gran_nodes;   // workgroups per CU the bound counts on; workgroups that own nodes; nodes per iteration of the granule region
  int service, n_wgrad;            // backward: workgroups beyond node_wgs (the head's loss, its parameter gradients); grid = node_wgs + service
};

// cus: CUs of the device.  multi_occupancy: workgroups per CU the iteration-major kernel of this direction (and filter shape)
// really gets, 0 .. 3 (read only for that form).  key8: spg_tune key 8 (1: no persistent form).  The bands of node counts that
// follow on an MI355X, two of which decline: DESIGN.md 4.23a.
inline SpgPxPlan spg_px_plan(const SpgPxGroups& groups, int R, bool backward, int cus, int multi_occupancy, int key8, const SpgPxHeadFacts& head) {
  const SpgPxPlan declined = {SPG_PX_DECLINED, 0, 0, 0, 0, 0};
  if (key8 == 1 || groups.n < 1 || R + 1 > SPG_PX_MAX_ITERS || R < 1) return declined;      // (2: only the iteration-major form is off, spg_px_plan_groups)
  const int mg = spg_px_max_group(groups);
  const bool multi = spg_px_is_multi(groups.n, mg);
  if (mg > SPG_PX_MAX_NODES && !multi) return declined;
  auto resident = [&](int wpc) { return wpc * (cus - SPG_PX_CU_MARGIN); };      // workgroups that are certainly resident at once
  auto wgs_for = [](int nodes) { return (nodes + 3) / 4; };                     // 4-wave workgroups, one node per wavefront
  if (multi) {      // the wavefronts of two workgroups per CU must cover the nodes, the granules fit the buffer
    auto covers = [](int wgs) { return (long)4 * wgs * SPG_PX_MULTI_NPW; };
    if (mg > covers(resident(2)) || (long)(R + 1) * mg > (long)SPG_PX_MAX_GROUPS * SPG_PX_MAX_ITERS * SPG_PX_MAX_NODES) return declined;
    // as many workgroups as stay resident with what the kernel really gets, no more than one wavefront per node
    const int wgs = wgs_for(mg) < resident(multi_occupancy) ? wgs_for(mg) : resident(multi_occupancy);
    if (multi_occupancy < 1 || covers(wgs) < mg) return declined;      // not resident enough
    return {SPG_PX_ITER_MAJOR, multi_occupancy, wgs, mg, 0, 0};
  }
  const int wpc = mg > SPG_PX_WG_NODES ? 2 : 1, node_wgs = wgs_for(mg), spare = resident(wpc) - node_wgs;
  if (spare < 0) return declined;
  SpgPxPlan pl = {wpc == 1 ? SPG_PX_ONE_PER_CU : SPG_PX_TWO_PER_CU, wpc, node_wgs, SPG_PX_MAX_NODES, 0, 0};
  if (backward && head.present && spare >= 1) {      // service workgroups on CUs the recurrence leaves idle; nobody waits for them
    pl.service = 1;                                  // the loss
    if (head.wgrad) {      // the classifier's parameter gradients: every wave of up to three service workgroups takes 64-column blocks
      const int nb = (head.nin + 63) / 64;
      pl.service = spare < 3 ? spare : 3;
      while (pl.service > 1 && 4 * (pl.service - 1) >= nb) --pl.service;
      pl.n_wgrad = pl.service;
    }
  }
  return pl;
}
