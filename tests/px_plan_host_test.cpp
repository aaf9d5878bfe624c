// Stand-alone host test of the launch plan of the one-launch GRU recurrences (csrc/spg_px_plan.h).  Built and run by
// tests/test_px_plan_host.py with -fsanitize=address,undefined.
//  (a) spg_px_plan_groups / spg_px_plan against a straight-line restatement of the code they replaced -- one function per old
//      function of the host section of csrc/spg_ecc.hip, with its own copies of the limits -- field by field over node counts,
//      devices, occupancies, iterations, spg_tune key 8, directions, filter shapes, round shapes and (backward) head facts;
//  (b) the bands of node counts on 256 CUs, written out;
//  (c) no plan leaves the residency bound, and an iteration-major plan covers its nodes;
//  (d) the rounds of the cases tests/test_gpu_ecc_edges.py::plan_rounds restates.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../superpoint_graph_amd/csrc/spg_px_plan.h"

#define REQUIRE(cond)                                                       \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

namespace {

// ---- the code before spg_px_plan.h, restated ----
const int OLD_WG_NODES = 1024, OLD_MAX_NODES = 2048, OLD_MAX_GROUPS = 8, OLD_MULTI_MAX_NODES = 16000;      // spg_ecc.h
const int OLD_MAX_ITERS = 16, OLD_MULTI_NPW = 8;                                                           // spg_ecc.hip

int old_cdiv(long a, long b) { return (int)((a + b - 1) / b); }      // spg_cdiv, spg_common.h

// spg_px_is_multi, spg_ecc.h
bool old_is_multi(int n_groups, int max_group) { return n_groups == 1 && max_group > OLD_MAX_NODES; }

// spg_px_plan_groups, spg_ecc.hip (spg_tune_get(SPG_TUNE_NO_PERSIST_ECC) -> key8)
bool old_plan_groups(int N, int n_parts, const int* part_ptr, int key8, SpgPxGroups* out) {
  const int cap = OLD_MAX_NODES;
  out->n = 0;
  if (N <= 0) return false;
  if (N <= cap) { out->n = 1; out->ptr[0] = 0; out->ptr[1] = N; return true; }
  auto big = [&]() -> bool {
    if (N > OLD_MULTI_MAX_NODES || key8 == 2) return false;
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
    if (b - start > cap) {
      if (out->n + 1 >= OLD_MAX_GROUPS) return big();
      out->ptr[++out->n] = a;
      start = a;
    }
  }
  out->ptr[++out->n] = N;
  return true;
}

// px_max_group, spg_ecc.hip
int old_max_group(const SpgPxGroups& g) {
  int m = 0;
  for (int k = 0; k < g.n; ++k) m = g.ptr[k + 1] - g.ptr[k] > m ? g.ptr[k + 1] - g.ptr[k] : m;
  return m;
}

// px_acquire, spg_ecc.hip: what it decided before it touched the runtime (the device queries succeed: cus)
bool old_acquire(const SpgPxGroups& groups, int R, int key8, int cus) {
  if (key8 == 1 || groups.n < 1 || R + 1 > OLD_MAX_ITERS || R < 1) return false;
  const int mg = old_max_group(groups);
  const bool multi = old_is_multi(groups.n, mg);
  if (mg > OLD_MAX_NODES && !multi) return false;
  const int wpc = mg > OLD_WG_NODES ? 2 : 1;
  if (multi) {
    if (mg > 4 * 2 * (cus - 4) * OLD_MULTI_NPW || (long)(R + 1) * mg > (long)OLD_MAX_GROUPS * OLD_MAX_ITERS * OLD_MAX_NODES) return false;
  } else if (old_cdiv(mg, 4) > wpc * (cus - 4)) return false;
  return true;
}

// px_spare_wgs, spg_ecc.hip
int old_spare_wgs(int node_wgs, int wpc, int cus) {
  const int spare = wpc * (cus - 4) - node_wgs;
  return spare > 0 ? spare : 0;
}

// px_multi_wgs, spg_ecc.hip
int old_multi_wgs(int nodes, int wpc, int cus) {
  const int cap = wpc * (cus - 4), need = old_cdiv(nodes, 4);
  return need < cap ? need : cap;
}

struct OldLaunch { bool launched, multi; int wpc, node_wgs, gran_nodes, service, n_wgrad; };      // grid = node_wgs + service
const OldLaunch OLD_FALLBACK = {false, false, 0, 0, 0, 0, 0};

// spg_launch_ecc_persist_fwd, spg_ecc.hip (occupancy = px_multi_wpc(matrix, false))
OldLaunch old_launch_fwd(const SpgPxGroups& groups, int R, int key8, int cus, int occupancy) {
  if (!old_acquire(groups, R, key8, cus)) return OLD_FALLBACK;
  const int mg = old_max_group(groups), wpc = mg <= OLD_WG_NODES ? 1 : 2;
  OldLaunch l = {true, false, wpc, old_cdiv(mg, 4), OLD_MAX_NODES, 0, 0};
  if (old_is_multi(groups.n, mg)) {
    const int wpc_m = occupancy;
    if (wpc_m < 1 || (long)4 * old_multi_wgs(mg, wpc_m, cus) * OLD_MULTI_NPW < mg) return OLD_FALLBACK;
    l.multi = true;
    l.wpc = wpc_m;
    l.node_wgs = old_multi_wgs(mg, wpc_m, cus);
    l.gran_nodes = mg;
  }
  return l;
}

// spg_launch_ecc_persist_bwd, spg_ecc.hip (occupancy = px_multi_wpc(matrix, true); wgrad = the conditions on head.dW,
// head_wgrad_done, C <= 16, key 6 and the alignment, in one)
OldLaunch old_launch_bwd(const SpgPxGroups& groups, int R, int key8, int cus, int occupancy, bool head, bool wgrad, int nin) {
  if (!old_acquire(groups, R, key8, cus)) return OLD_FALLBACK;
  const int mg = old_max_group(groups), wpc = mg <= OLD_WG_NODES ? 1 : 2;
  OldLaunch l = {true, false, wpc, old_cdiv(mg, 4), OLD_MAX_NODES, 0, 0};
  if (old_is_multi(groups.n, mg)) {
    const int wpc_m = occupancy;
    if (wpc_m < 1 || (long)4 * old_multi_wgs(mg, wpc_m, cus) * OLD_MULTI_NPW < mg) return OLD_FALLBACK;
    l.multi = true;
    l.wpc = wpc_m;
    l.node_wgs = old_multi_wgs(mg, wpc_m, cus);
    l.gran_nodes = mg;
    return l;
  }
  int service = 0;
  if (head) {
    const int spare = old_spare_wgs(l.node_wgs, wpc, cus);
    if (spare >= 1) service = 1;
    if (spare >= 1 && wgrad) {
      const int nb = (nin + 63) / 64;
      service = spare < 3 ? spare : 3;
      while (service > 1 && 4 * (service - 1) >= nb) --service;
      l.n_wgrad = service;
    }
  }
  l.service = service;
  return l;
}

// ---- the comparison ----
SpgPxForm form_of(const OldLaunch& l) {
  return !l.launched ? SPG_PX_DECLINED : l.multi ? SPG_PX_ITER_MAJOR : l.wpc == 1 ? SPG_PX_ONE_PER_CU : SPG_PX_TWO_PER_CU;
}

long g_plans = 0;

void same(const SpgPxPlan& pl, const OldLaunch& l, int cus) {
  ++g_plans;
  REQUIRE(pl.form == form_of(l));
  REQUIRE(pl.wpc == l.wpc && pl.node_wgs == l.node_wgs && pl.gran_nodes == l.gran_nodes);
  REQUIRE(pl.service == l.service && pl.n_wgrad == l.n_wgrad);
  if (pl.form == SPG_PX_DECLINED) return;
  // (c)
  REQUIRE(pl.node_wgs >= 1 && pl.node_wgs + pl.service <= pl.wpc * (cus - SPG_PX_CU_MARGIN));
  REQUIRE(pl.n_wgrad <= pl.service);
  if (pl.form == SPG_PX_ITER_MAJOR) REQUIRE((long)4 * pl.node_wgs * SPG_PX_MULTI_NPW >= pl.gran_nodes);      // gran_nodes = the nodes of the one round
}

// part_ptr of round shape `shape` for a graph of N nodes; n_parts = size - 1 (an empty vector: components unknown)
const int N_SHAPES = 8;
std::vector<int> part_ptr_of(int shape, int N) {
  auto equal = [&](int k) {
    std::vector<int> p(k + 1);
    for (int i = 0; i <= k; ++i) p[i] = (int)((long)N * i / k);
    return p;
  };
  switch (shape) {
    case 0: return {};                                      // one round (or, above SPG_PX_MAX_NODES, one group)
    case 1: return equal(2);                                // 2 rounds where the halves fit a round
    case 2: return equal(8);                                // up to 8 rounds
    case 3: return equal(9);                                // 9 rounds above 9 * 1024 nodes: too many
    case 4: return {0, N < 2049 ? N : 2049, N};             // a part above a round
    case 5: { std::vector<int> p = equal(8); p[0] = 1; return p; }          // first != 0: one group, not the rounds its parts would pack into
    case 6: { std::vector<int> p = equal(8); p[8] = N - 1; return p; }      // last != N: the same
    default: return {0, 1500, 700, N};                      // decreasing, behind a part that fits a round: no rounds at all
  }
}

bool same_rounds(const SpgPxGroups& a, const SpgPxGroups& b) {
  if (a.n != b.n) return false;
  for (int k = 0; k <= a.n && a.n > 0; ++k)
    if (a.ptr[k] != b.ptr[k]) return false;
  return true;
}

// every input of the plan but the rounds and key 8.  The occupancy stands for px_multi_wpc(matrix, direction) of the launchers: the
// filter shape enters the plan through it alone, so all four values in both directions cover `matrix` on and off.
void sweep_plans(const SpgPxGroups& g_new, const SpgPxGroups& g_old, int key8) {
  const int CUS[] = {8, 64, 104, 256, 304}, RS[] = {0, 1, 15, 16}, NINS[] = {32, 64, 352, 512};
  for (int cus : CUS)
    for (int occupancy = 0; occupancy <= 3; ++occupancy)
      for (int R : RS) {
        const OldLaunch fwd = old_launch_fwd(g_old, R, key8, cus, occupancy);
        same(spg_px_plan(g_new, R, false, cus, occupancy, key8, SpgPxHeadFacts{false, false, 0}), fwd, cus);
        same(spg_px_plan(g_new, R, false, cus, occupancy, key8, SpgPxHeadFacts{true, true, 512}), fwd, cus);      // the forward reads nothing of the head
        for (int head = 0; head <= 1; ++head)
          for (int wgrad = 0; wgrad <= 1; ++wgrad)
            for (int nin : NINS)
              same(spg_px_plan(g_new, R, true, cus, occupancy, key8, SpgPxHeadFacts{head != 0, wgrad != 0, nin}),
                   old_launch_bwd(g_old, R, key8, cus, occupancy, head != 0, wgrad != 0, nin), cus);
      }
}

void sweep() {
  for (int N = 1; N <= 17000; ++N)
    for (int key8 = 0; key8 <= 2; ++key8) {
      std::vector<SpgPxGroups> swept;
      for (int shape = 0; shape < N_SHAPES; ++shape) {
        const std::vector<int> parts = part_ptr_of(shape, N);
        const int n_parts = parts.empty() ? 0 : (int)parts.size() - 1;
        SpgPxGroups g_new, g_old;
        const bool ok_new = spg_px_plan_groups(N, n_parts, parts.empty() ? nullptr : parts.data(), key8, &g_new);
        const bool ok_old = old_plan_groups(N, n_parts, parts.empty() ? nullptr : parts.data(), key8, &g_old);
        REQUIRE(ok_new == ok_old && same_rounds(g_new, g_old));
        if (!ok_new) g_new.n = g_old.n = 0;      // what a caller that ignores the result would hand on: no rounds
        REQUIRE(spg_px_max_group(g_new) == old_max_group(g_old));
        REQUIRE(spg_px_groups_multi(g_new) == old_is_multi(g_old.n, old_max_group(g_old)));
        // the plan is a pure function of the rounds: a shape that gives the rounds of an earlier one (up to SPG_PX_MAX_NODES
        // nodes every shape gives the one round) has been swept with it
        bool again = false;
        for (const SpgPxGroups& g : swept) again = again || same_rounds(g, g_new);
        if (again) continue;
        swept.push_back(g_new);
        sweep_plans(g_new, g_old, key8);
      }
    }
}

// (b) the form of a graph of N nodes whose components are unknown, 10 iterations, on 256 CUs
SpgPxForm form_256(int N, int occupancy, bool backward) {
  SpgPxGroups g;
  if (!spg_px_plan_groups(N, 0, nullptr, 0, &g)) return SPG_PX_DECLINED;
  return spg_px_plan(g, 10, backward, 256, occupancy, 0, SpgPxHeadFacts{false, false, 0}).form;
}

void bands() {
  for (int backward = 0; backward <= 1; ++backward)
    for (int N = 1; N <= 17000; ++N) {
      const SpgPxForm small = N <= 1008 ? SPG_PX_ONE_PER_CU : N <= 1024 ? SPG_PX_DECLINED : N <= 2016 ? SPG_PX_TWO_PER_CU : SPG_PX_DECLINED;
      for (int occupancy = 2; occupancy <= 3; ++occupancy)
        REQUIRE(form_256(N, occupancy, backward != 0) == (N <= 2048 ? small : N <= 16000 ? SPG_PX_ITER_MAJOR : SPG_PX_DECLINED));
      REQUIRE(form_256(N, 1, backward != 0) == (N <= 2048 ? small : N <= 8064 ? SPG_PX_ITER_MAJOR : SPG_PX_DECLINED));
      REQUIRE(form_256(N, 0, backward != 0) == (N <= 2048 ? small : SPG_PX_DECLINED));
    }
}

// (d) node counts of the rounds, as tests/test_gpu_ecc_edges.py::plan_rounds gives them (an empty list: None)
void rounds_are(int N, const std::vector<int>& part_ptr, const std::vector<int>& want) {
  SpgPxGroups g;
  const bool ok = spg_px_plan_groups(N, part_ptr.empty() ? 0 : (int)part_ptr.size() - 1, part_ptr.empty() ? nullptr : part_ptr.data(), 0, &g);
  REQUIRE(ok == !want.empty());
  if (!ok) return;
  REQUIRE(g.n == (int)want.size() && g.ptr[0] == 0);
  for (int k = 0; k < g.n; ++k) REQUIRE(g.ptr[k + 1] - g.ptr[k] == want[k]);
}

void rounds() {
  for (int N : {3, 5, 200, 1008, 1024, 1025, 2048}) rounds_are(N, {0, N}, {N});      // the ladder graphs: one round
  rounds_are(2049, {0, 2049}, {2049});                                               // one group above a round
  rounds_are(2200, {0, 700, 1600, 2200}, {1600, 600});                               // 'scenes' = (700, 900, 600): 2 rounds
  rounds_are(5000, {}, {5000});
  rounds_are(16000, {}, {16000});
  rounds_are(16001, {}, {});
  rounds_are(4096, {0, 2048, 4096}, {2048, 2048});
  rounds_are(16384, {0, 2048, 4096, 6144, 8192, 10240, 12288, 14336, 16384}, {2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048});
  rounds_are(18432, {0, 2048, 4096, 6144, 8192, 10240, 12288, 14336, 16384, 18432}, {});      // 9 rounds above the one-group limit
  rounds_are(12000, {0, 1500, 3000, 4500, 6000, 7500, 9000, 10500, 12000}, {1500, 1500, 1500, 1500, 1500, 1500, 1500, 1500});
  rounds_are(13500, {0, 1500, 3000, 4500, 6000, 7500, 9000, 10500, 12000, 13500}, {13500});      // 9 rounds: one group instead
  rounds_are(3000, {0, 2500, 3000}, {3000});                                         // a part above a round: one group
  rounds_are(4096, {1, 2048, 4096}, {4096});                                         // first != 0: components unknown, one group
  rounds_are(4096, {0, 2048, 4095}, {4096});                                         // last != N: the same
  rounds_are(3000, {0, 1500, 700, 3000}, {});                                       // decreasing: malformed, not one group
}

}  // namespace

int main() {
  rounds();
  bands();
  sweep();
  std::printf("px_plan_host_test: ok (%ld plans compared)\n", g_plans);
  return 0;
}
