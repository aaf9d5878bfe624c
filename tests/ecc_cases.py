"""Case builders and float64 references for the edge-conditioned graph convolution (csrc/spg_ecc.hip, csrc/spg_eccnet.hip) at
its DEGREE thresholds: the in-edge aggregation (spg_aggregate_node), the persistent / several-nodes-per-wavefront / per-iteration
forms of the GRU / LSTM recurrence, the reverse-CSR build and the edge weight gradient.  Plain module (no test in it):
tests/test_ecc_cases.py checks the graphs, admits the cases and probes the knobs on the CPU, tests/test_gpu_ecc_edges.py runs the
device against the references.

THE LADDER GRAPH  ladder_graph(n, seed) -> (idxn i64 [E], degs i64 [n], parts), edges sorted by target (stable), as set_batch
delivers them.  200 ROLES are placed on the n >= 200 nodes by a seeded permutation (ladder_nodes(n, seed)[role] is the node of a
role), except that the in-degree-100 hub is the LAST node (alone in the last workgroup at n = 1025 and 2049) and the out-degree-100
hub the one before it.  Roles:

  0 .. 19   in-degree  LADDER[k] = 0 1 2 3 4 5 6 7 8 9 11 12 13 31 32 33 63 64 65 100, distinct sources from the pool; out-degree 1
 20 .. 39   out-degree LADDER[k], distinct targets in the pool; in-degree 1
 40         in-hub AND out-hub: 36 in-edges from, 36 out-edges into the pool
 41         a self-loop (41 -> 41) and two more in-edges; out-degree 1 (the loop)
 42 -> 43   a TRIPLE edge (42: in 1, out 3; 43: in 3, out 1)
 44         in-degree 40, every source is role 45 (45: in 1, out 40); out-degree 1
 46         no out-edges (in-degree 2)
 47 .. 59   isolated
 60 .. 199  the pool: a ring over 60 .. 159 plus whatever the roles above draw from it (degrees not pinned)
 >= 200     isolated

so E = 1202 whatever n is.  What each rung guards (csrc/spg_ecc.hip):
  0                 invdeg = 0, exact-zero rows;   1 2 3 | 4 | 5: the 4-edge batches of spg_aggregate_node (tail clamp + `on` mask)
  7 | 8 | 9         UNR = 8 of the per-iteration backward helper (over out-edges) and two full 4-batches
  1 | 2 | 3         SPG_PX_KMAX2B = 2 (backward, two workgroups per CU);   5 | 6 | 7: SPG_PX_KMAX2 = 6
  11 | 12 | 13      SPG_PX_KMAX1 = 12 (one workgroup per CU)
  31 | 32 | 33      SPG_PX_CH = 32: one gather pass / a second one;   63 | 64 | 65: two passes / a third;   100: four passes
The out-degree ladder guards the same constants in the backward (odeg, rev_eid) and the insertion sort of spg_graph_revsort_kernel.
Sizes: n = 200 and 1008 (persistent launch, one workgroup per CU; 1008 = 4 (256 - 4) is the largest graph whose 252 workgroups the
residency bound of spg_px_plan admits on the 256 CUs of an MI355X, and its last workgroup is full), 1024 (inside the band 1009 .. 1024
that the launcher sends to the PER-ITERATION launches on this part: 256 workgroups exceed the bound and two per CU start at 1025 only),
1025 (two per CU: KMAX 6 / 2), 2049 (one group above 2048 nodes: the iteration-major kernels; at this size a wavefront owns one node
in the forward and at most two in the backward -- SPG_PX_MULTI_NPW = 8 nodes per wavefront are reached only by the bit-identity tests
at 5000 and 10000 nodes); scenes = (700, 900, 600) puts the ladder in the LAST scene (group and node offsets != 0, GROUPS = true), the
other scenes hold a ring each; n = 3 and 5 (tiny_graph) are a partial first workgroup with a self-loop, a repeated edge and in-degrees
5, 13.

REFERENCES are the float64 evaluation of oracle/spg_oracle.py: ecc_forward / ecc_backward for the operator, graph_network_forward
and torch autograd for the module.  Every evaluator takes a dtype (float64: the reference; float32 on the CPU: the admission
figure).  Nothing here is derived from what the device returns.

BOUNDS.  conftest.assert_elementwise with its defaults, |a - ref| <= 1e-4 |ref| + 1e-5 max|ref| for every element; for the
operator the floor is taken per ROW of out / grad_x and per EDGE (filter) of grad_w (row_bound_ratio / assert_row_bound), so that a
hub's 1/deg scale cannot hide behind degree-1 rows; float64 runs: 1e-13 of the row's maximum per element.  A case is admitted only if
its float32 CPU evaluation stays within ADMIT = 0.25 of the bound on every compared tensor.  No rung had to be dropped.

RELU NEAR-TIES of the filter network: the float32 side's decisions are handed to the float64 backward (`dec`), exactly as
tests/test_gpu_baseline_parity.py::_decision_conditioned does; `out` is always judged against the unconditioned reference.

KNOBS (keyword switches, all off by default; each restates one plausible kernel mistake, see KNOBS below).  With any knob the
operator is evaluated by a restatement (_KnobEcc) whose all-off form equals the oracle bit for bit.  A knob acts on every node it
applies to, so tests/test_ecc_cases.py shows that the bound SEES such a mistake; that a single rung cannot hide is the work of the
per-row / per-edge floor: a wrong row is judged against its own largest value, whatever the other rows hold."""
import functools

import numpy as np
import torch

from oracle import spg_oracle as O
from op_cases import ADMIT, ATOL_FRAC, RTOL, assert_bound, bound_ratio, worst  # noqa: F401  (re-exported for the tests)

LADDER = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 31, 32, 33, 63, 64, 65, 100)
IN0, OUT0, BOTH, SELF, TRI_SRC, TRI_DST, MONO_HUB, MONO_SRC, SINK = 0, 20, 40, 41, 42, 43, 44, 45, 46
POOL0, RING1, MIN_N = 60, 160, 200
BOTH_DEG, MONO_DEG = 36, 40
SIZES = (200, 1008, 1024, 1025, 2049)
SCENES = (700, 900, 600)
TINY = (3, 5)
F64_TOL = 1e-13

# name -> keyword arguments of the evaluators; ORDER_ONLY must stay inside the bound, every other one must leave it somewhere
KNOBS = {
    'tail of a 4-edge batch dropped': dict(tail='drop'),
    'tail of a 4-edge batch counted again (clamp without the mask)': dict(tail='clamp'),
    'edges KMAX .. min(deg, 32) - 1 skipped, KMAX = 12': dict(skip_from=12),
    'edges KMAX .. min(deg, 32) - 1 skipped, KMAX = 6': dict(skip_from=6),
    'edges KMAX .. min(deg, 32) - 1 skipped, KMAX = 2': dict(skip_from=2),
    'later passes reuse the sources of the first pass': dict(reuse_first_pass=True),
    'mean divides by deg + 1': dict(divisor='deg+1'),
    'a repeated edge is counted once': dict(dedup=True),
    'a self-loop reads the state being written': dict(self_loop_new=True),
    'out-edge lists truncated at 32 in the backward': dict(bwd_out_limit=32),
}
ORDER_ONLY = {'rev_eid lists unsorted (sum order only)': dict(rev_unsorted=True)}
MODULE_ONLY = ('a self-loop reads the state being written',)


# =====================================================================================================================
# graphs
# =====================================================================================================================
def _role_edges(n, seed):
    """-> (edges i64 [E, 2] (source, target) over ROLE numbers, in a shuffled order; place i64 [n]: role -> node)."""
    assert n >= MIN_N
    rng = np.random.default_rng(1000 * n + seed)
    pool = np.arange(POOL0, MIN_N)
    pick = lambda k: rng.choice(pool, size=k, replace=False)
    ed = []
    for k, d in enumerate(LADDER):
        ed += [(int(s), IN0 + k) for s in pick(d)] + [(IN0 + k, int(pick(1)[0]))]
        ed += [(OUT0 + k, int(t)) for t in pick(d)] + [(int(pick(1)[0]), OUT0 + k)]
    ed += [(int(s), BOTH) for s in pick(BOTH_DEG)] + [(BOTH, int(t)) for t in pick(BOTH_DEG)]
    ed += [(SELF, SELF)] + [(int(s), SELF) for s in pick(2)]
    ed += [(TRI_SRC, TRI_DST)] * 3 + [(int(pick(1)[0]), TRI_SRC), (TRI_DST, int(pick(1)[0]))]
    ed += [(MONO_SRC, MONO_HUB)] * MONO_DEG + [(int(pick(1)[0]), MONO_SRC), (MONO_HUB, int(pick(1)[0]))]
    ed += [(int(s), SINK) for s in pick(2)]
    ed += [(i, POOL0 + (i + 1 - POOL0) % (RING1 - POOL0)) for i in range(POOL0, RING1)]
    ed = np.asarray(ed, dtype=np.int64)
    ed = ed[rng.permutation(len(ed))]
    place = rng.permutation(n).astype(np.int64)

    def force(role, node):                       # the role sits on `node`; whoever sat there takes the role's old node
        j = int(np.nonzero(place == node)[0][0])
        place[j], place[role] = place[role], node
    force(IN0 + len(LADDER) - 1, n - 1)
    force(OUT0 + len(LADDER) - 1, n - 2)
    return ed, place


def _sorted_by_target(edges, n):
    order = np.argsort(edges[:, 1], kind='stable')
    e = edges[order]
    return torch.from_numpy(e[:, 0].copy()), torch.from_numpy(np.bincount(e[:, 1], minlength=n).astype(np.int64))


def _ring(n0, k):
    return np.asarray([(n0 + i, n0 + (i + 1) % k) for i in range(k)], dtype=np.int64)


def ladder_graph(n, seed=0, scenes=None):
    """-> (idxn, degs, parts).  scenes: node counts of a multi-scene batch (n = their sum); the ladder is the LAST scene."""
    if scenes is None:
        ed, place = _role_edges(n, seed)
        edges, parts = place[ed], [0, n]
    else:
        assert n == sum(scenes)
        off = np.concatenate([[0], np.cumsum(scenes)])
        ed, place = _role_edges(scenes[-1], seed)
        edges = np.concatenate([_ring(int(off[s]), 60) for s in range(len(scenes) - 1)] + [place[ed] + off[-2]])
        parts = [int(v) for v in off]
    idxn, degs = _sorted_by_target(edges, n)
    return idxn, degs, parts


def ladder_nodes(n, seed=0, scenes=None):
    """role -> node (i64 [200]) of ladder_graph(n, seed, scenes)."""
    if scenes is None:
        return _role_edges(n, seed)[1][:MIN_N]
    return _role_edges(scenes[-1], seed)[1][:MIN_N] + (n - scenes[-1])


def ladder_degrees():
    """role -> (in-degree, out-degree) for the roles whose degrees are pinned (0 .. 59)."""
    d = {}
    for k, v in enumerate(LADDER):
        d[IN0 + k], d[OUT0 + k] = (v, 1), (1, v)
    d.update({BOTH: (BOTH_DEG, BOTH_DEG), SELF: (3, 1), TRI_SRC: (1, 3), TRI_DST: (3, 1), MONO_HUB: (MONO_DEG, 1), MONO_SRC: (1, MONO_DEG),
              SINK: (2, 0)})
    d.update({r: (0, 0) for r in range(SINK + 1, POOL0)})
    return d


TINY_IN = {3: (5, 1, 0), 5: (5, 1, 0, 13, 0)}
TINY_OUT = {3: (2, 2, 2), 5: (5, 5, 5, 2, 2)}


def tiny_graph(n):
    """n = 3: node 0 has in-degree 5 (its own loop, 1 and 2 twice each), node 1 in-degree 1, node 2 none; n = 5 adds node 3 with
    in-degree 13 (sources 0 1 2 3 4 0 1 ...: a loop and repeats) and node 4 without in-edges."""
    ed = [(0, 0), (1, 0), (2, 0), (1, 0), (2, 0), (0, 1)]
    if n == 5:
        ed += [(i % 5, 3) for i in range(13)]
    idxn, degs = _sorted_by_target(np.asarray(ed, dtype=np.int64), n)
    return idxn, degs, [0, n]


@functools.lru_cache(maxsize=None)
def graph(key):
    """key: an int n (ladder or tiny graph) or the string 'scenes'."""
    if key == 'scenes':
        return ladder_graph(sum(SCENES), 0, SCENES)
    return tiny_graph(key) if key in TINY else ladder_graph(key, 0)


GRAPH_KEYS = TINY + SIZES + ('scenes',)


# =====================================================================================================================
# the operator with knobs
# =====================================================================================================================
def _edge_plan(idxn, degs, tail=None, skip_from=None, reuse_first_pass=False, dedup=False, bwd_out_limit=None, rev_unsorted=False):
    """Per-edge restatement of the mistakes: (source actually read, forward multiplicity, backward multiplicity of the edge in
    grad_x, order in which grad_x is accumulated)."""
    n, E = int(degs.numel()), int(idxn.numel())
    rp = torch.from_numpy(O.csr_by_target(degs.numpy()))
    dst = torch.repeat_interleave(torch.arange(n), degs)
    pos = torch.arange(E) - rp[dst]
    deg = degs[dst]
    mf, mb, src = torch.ones(E, dtype=torch.float64), torch.ones(E, dtype=torch.float64), idxn.clone()
    if tail == 'drop':
        mf[pos >= (deg // 4) * 4] = 0.0
    elif tail == 'clamp':
        last = (pos == deg - 1) & (deg % 4 != 0)
        mf[last] = (1 + (4 - deg % 4))[last].double()
    if skip_from is not None:
        mf[(pos >= skip_from) & (pos < 32)] = 0.0
    if reuse_first_pass:
        src = idxn[rp[dst] + pos % 32]
    if dedup:
        seen = set()
        for e in range(E):
            k = (int(idxn[e]), int(dst[e]))
            if k in seen:
                mf[e] = 0.0
            seen.add(k)
    order = torch.arange(E)
    if bwd_out_limit is not None or rev_unsorted:
        rrp, rev = O.csr_by_source(idxn.numpy(), n)
        rank = torch.empty(E, dtype=torch.int64)
        rank[torch.from_numpy(rev)] = torch.arange(E) - torch.from_numpy(rrp)[idxn[torch.from_numpy(rev)]]
        if bwd_out_limit is not None:
            mb[rank >= bwd_out_limit] = 0.0
        if rev_unsorted:
            order = torch.from_numpy(np.random.default_rng(5).permutation(E))
    return src, mf, mb, order


class _KnobEcc(torch.autograd.Function):
    """oracle.spg_oracle.ecc_forward / ecc_backward with the per-edge plan above (all off: the same expressions in the same order).
    alt: (state of the iteration being written, bool mask of the edges that read it) or None."""

    @staticmethod
    def forward(ctx, x, w, idxn, degs, idxe, plan, divisor, alt):
        src, mf, mb, order = plan
        n = degs.numel()
        dst = torch.repeat_interleave(torch.arange(n), degs)
        sel = x.index_select(0, src)
        if alt is not None:
            sel = torch.where(alt[1].unsqueeze(1), alt[0].index_select(0, src), sel)
        ww = w if idxe is None else w.index_select(0, idxe)
        prod = torch.bmm(sel.unsqueeze(1), ww).squeeze(1) if w.dim() == 3 else sel * ww
        out = torch.zeros(n, prod.shape[1], dtype=x.dtype)
        out.index_add_(0, dst, prod * mf.to(x.dtype).unsqueeze(1))
        div = (degs + 1 if divisor == 'deg+1' else degs.clamp(min=1)).to(x.dtype)
        ctx.save_for_backward(x, w, sel)
        ctx.meta = (idxn, degs, idxe, plan, div, dst)
        return out / div.unsqueeze(1)

    @staticmethod
    def backward(ctx, grad_out):
        x, w, sel = ctx.saved_tensors
        idxn, degs, idxe, (src, mf, mb, order), div, dst = ctx.meta
        g = grad_out.index_select(0, dst) * mf.to(x.dtype).unsqueeze(1) / div.index_select(0, dst).unsqueeze(1)
        ww = w if idxe is None else w.index_select(0, idxe)
        if w.dim() == 3:
            gw_e = sel.unsqueeze(2) * g.unsqueeze(1)
            gsel = torch.bmm(g.unsqueeze(1), ww.transpose(1, 2)).squeeze(1)
        else:
            gw_e = sel * g
            gsel = g * ww
        gw = gw_e if idxe is None else torch.zeros_like(w).index_add_(0, idxe, gw_e)
        gsel = gsel * mb.to(x.dtype).unsqueeze(1)
        gx = torch.zeros_like(x)
        gx.index_add_(0, src.index_select(0, order), gsel.index_select(0, order))
        return gx, gw, None, None, None, None, None, None


def _split_knobs(knobs):
    k = dict(knobs)
    divisor, self_loop_new = k.pop('divisor', None), k.pop('self_loop_new', False)
    return k, divisor, self_loop_new


# ---------------------------------------------------------------------------------------------------------------------
# operator cases
# ---------------------------------------------------------------------------------------------------------------------
OP_SHAPES = {'32x32 matrix': (32, 32, True), '32 vector': (32, 32, False), '10x15 matrix': (10, 15, True)}
OP_SCALES = (1.0, 1e-3, 1e3)


@functools.lru_cache(maxsize=None)
def op_case(gkey, shape, scale, shared=False):
    """float32 inputs of one operator case: x [n, cin] * scale, filters w ([E, cin, cout] / [E, c]; shared: [E // 3, cin, cout] picked by
    idxe), the upstream gradient [n, cout]."""
    cin, cout, matrix = OP_SHAPES[shape]
    idxn, degs, _ = graph(gkey)
    n, E = int(degs.numel()), int(idxn.numel())
    g = torch.Generator().manual_seed(11 + 7 * n + cin + 3 * int(matrix))
    x = torch.randn(n, cin, generator=g) * scale
    nw = max(E // 3, 1) if shared else E
    w = torch.randn(*((nw, cin, cout) if matrix else (nw, cout)), generator=g) / (cin ** 0.5 if matrix else 1.0)
    go = torch.randn(n, cout, generator=g)
    idxe = torch.randint(0, nw, (E,), generator=g) if shared else None
    return dict(name=f'operator {shape}, graph {gkey}, x * {scale:g}' + (', shared filters' if shared else ''), gkey=gkey, x=x, w=w, go=go, idxe=idxe)


def op_eval(case, dtype=torch.float64, **knobs):
    """-> {out, grad_x, grad_w} of the operator in `dtype` on the CPU; without knobs: oracle.spg_oracle.ecc_forward / ecc_backward."""
    idxn, degs, _ = graph(case['gkey'])
    x, w, go = [case[k].to(dtype) for k in ('x', 'w', 'go')]
    if not knobs:
        out = O.ecc_forward(x, w, idxn, degs, case['idxe'])
        gx, gw = O.ecc_backward(x, w, go, idxn, degs, case['idxe'])
        return {'out': out, 'grad_x': gx, 'grad_w': gw}
    k, divisor, _ = _split_knobs(knobs)
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out = _KnobEcc.apply(x, w, idxn, degs, case['idxe'], _edge_plan(idxn, degs, **k), divisor, None)
    out.backward(go)
    return {'out': out.detach(), 'grad_x': x.grad, 'grad_w': w.grad}


def _rows(v):
    v = (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).detach().double().cpu()
    return v.reshape(v.shape[0], -1) if v.dim() > 1 else v.reshape(-1, 1)


def row_bound_ratio(a, ref, rtol=RTOL, atol_frac=ATOL_FRAC):
    """bound_ratio with the floor taken per row (dimension 0: a node of out / grad_x, an edge or filter of grad_w):
    -> (worst |a - ref|, worst |a - ref| / (rtol |ref| + atol_frac max_row|ref|)); inf where an element is off although its bound is 0."""
    a, ref = _rows(a), _rows(ref)
    if a.shape != ref.shape or bool(torch.isnan(a).any()) or bool(torch.isnan(ref).any()):
        return float('inf'), float('inf')
    if ref.numel() == 0:
        return 0.0, 0.0
    err = (a - ref).abs()
    bound = rtol * ref.abs() + atol_frac * ref.abs().max(1, keepdim=True).values
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(err.max()), float(ratio.max())


def assert_row_bound(a, ref, what, rtol=RTOL, atol_frac=ATOL_FRAC):
    """conftest.assert_elementwise row by row (each row judged against its own largest reference value), NaN nowhere."""
    a2, r2 = _rows(a), _rows(ref)
    assert a2.shape == r2.shape, (what, a2.shape, r2.shape)
    assert not bool(torch.isnan(a2).any()), f'{what}: NaN'
    bound = rtol * r2.abs() + atol_frac * r2.abs().max(1, keepdim=True).values
    excess = (a2 - r2).abs() - bound
    if excess.numel():
        row = int(excess.max(1).values.argmax())
        assert float(excess.max()) <= 0.0, (f'{what}: row {row} exceeds rtol {rtol} + {atol_frac} * max|ref row| by {float(excess.max()):.3e} '
                                            f'(row maximum {float(r2[row].abs().max()):.3e})')


def measure_rows(got, ref, **kw):
    return {k: row_bound_ratio(got[k], ref[k], **kw) for k in ref}


# =====================================================================================================================
# the recurrent module
# =====================================================================================================================
FNET = [13, 32, 128, 64]                     # edge features -> filter network widths; orthogonal init, no last-layer bias, BatchNorm at 2
CONFIGS = {'matrix': 'gru_10_0', 'vector': 'gru_4_1', 'plain': 'gru_3_0_0_0_1', 'lstm': 'lstm_3_0'}
NOISE = {c: ('ecc.0._fnet.4.bias',) for c in CONFIGS}        # pinned by tests/test_ecc_cases.py


def module_spec(config):
    return O.ModelSpec(model_config=CONFIGS[config])


@functools.lru_cache(maxsize=None)
def module_state(config):
    """The float32 state_dict of graphnet.GraphNetwork for a configuration (its own initialisation, seed 7), keys prefixed 'ecc.'."""
    from superpoint_graph_amd.learning import graphnet
    with torch.random.fork_rng():
        torch.manual_seed(7)
        net = graphnet.GraphNetwork(CONFIGS[config], 32, list(FNET), 1, 0, 2, 30000, use_pyg=0, cuda=1)
    return {'ecc.' + k: v.detach().clone() for k, v in net.state_dict().items()}


@functools.lru_cache(maxsize=None)
def module_case(config, gkey, training=True):
    idxn, degs, parts = graph(gkey)
    n, E = int(degs.numel()), int(idxn.numel())
    g = torch.Generator().manual_seed(23 + n)
    x = torch.randn(n, 32, generator=g)
    ef = torch.randn(E, 13, generator=g)
    R = int(CONFIGS[config].split('_')[1])
    go = torch.randn(n, 32 * (R + 1), generator=g)
    return dict(name=f'module {config} ({CONFIGS[config]}), graph {gkey}, ' + ('train' if training else 'eval'), config=config, gkey=gkey,
                training=training, x=x, edgefeats=ef, go=go, parts=parts)


def _module_forward_knobs(x, ef, idxn, degs, spec, P, training, dec, rec, knobs):
    """oracle.spg_oracle.graph_network_forward for a single gru / lstm token, the operator replaced by _KnobEcc."""
    (d, kind, payload), = O.parse_model_config(spec.model_config, 32)
    rs, pfx = payload[1], f'ecc.{d}'
    k, divisor, self_loop_new = _split_knobs(knobs)
    plan = _edge_plan(idxn, degs, **k)
    w = O.fnet_forward(ef.to(x.dtype), spec, 32 if rs.vv else 1024, P, training, None, pfx + '._fnet', dec, rec)
    if not rs.vv:
        w = w.view(-1, 32, 32)
    loops = idxn == torch.repeat_interleave(torch.arange(degs.numel()), degs)
    hx, hxs = x, [x]
    cx = torch.zeros_like(x) if rs.kind == 'lstm' else None

    def cell(inp, hx, cx):
        if rs.kind == 'lstm':
            return O.lstm_cell_ex(inp, (hx, cx), P, pfx + '._cell', rs.layernorm, rs.ingate)
        return O.gru_cell_ex(inp, hx, P, pfx + '._cell', rs.layernorm, rs.ingate), None
    for _ in range(rs.nrepeats):
        inp = _KnobEcc.apply(hx, w, idxn, degs, None, plan, divisor, None)
        hy, cy = cell(inp, hx, cx)
        if self_loop_new:                       # the loop edge reads hy of its node: one more evaluation with that row swapped in
            inp = _KnobEcc.apply(hx, w, idxn, degs, None, plan, divisor, (hy, loops))
            hy, cy = cell(inp, hx, cx)
        hx, cx = hy, cy
        hxs.append(hx)
    return torch.cat(hxs, 1) if rs.cat_all else hx


def module_eval(case, dtype=torch.float64, dec=None, rec=None, **knobs):
    """-> {out, 'grad x', 'grad <parameter>' ...} in `dtype` on the CPU (evaluation mode: out only).  Without knobs:
    oracle.spg_oracle.graph_network_forward under torch autograd.  dec / rec: the ReLU decision hooks of the filter network."""
    idxn, degs, _ = graph(case['gkey'])
    spec = module_spec(case['config'])
    P = {k: (v.to(dtype).clone().requires_grad_(True) if (O.is_param_key(k) and v.is_floating_point()) else v.clone())
         for k, v in module_state(case['config']).items()}
    x = case['x'].to(dtype).clone().requires_grad_(case['training'])
    ef = case['edgefeats'].to(dtype)
    if knobs:
        out = _module_forward_knobs(x, ef, idxn, degs, spec, P, case['training'], dec, rec, knobs)
    else:
        out = O.graph_network_forward(x, ef, idxn, degs, spec, P, case['training'], dec=dec, rec=rec)
    res = {'out': out.detach()}
    if case['training']:
        out.backward(case['go'].to(dtype))
        res['grad x'] = x.grad
        for k, v in P.items():
            if v.requires_grad:
                res['grad ' + k] = v.grad if v.grad is not None else torch.zeros_like(v)
    return res


def param_grads(res):
    """{parameter key: gradient} of a module_eval result (what conftest.noise_grad reads)."""
    return {k[5:]: v for k, v in res.items() if k.startswith('grad ecc.')}


def compared(case, ref):
    """The tensors of a module case that are judged: out, grad x and every parameter gradient that conftest.noise_grad does not
    exclude on the float64 reference."""
    from conftest import noise_grad
    pg = param_grads(ref)
    return [k for k in ref if not (k.startswith('grad ecc.') and noise_grad(k[5:], pg))]


def decisions(rec):
    """ReLU decisions (bool masks) of recorded pre-activations."""
    return {k: v > 0 for k, v in rec.items()}


def check_near_ties(dec, rec_ref, tie_tol=1e-4):
    """The project's rule (tests/test_gpu_baseline_parity.py): a decision may differ from the float64 reference's own only where
    |z_ref| <= tie_tol * the layer's largest value, and at most 10 * tie_tol * numel of them.  -> number of differing decisions."""
    total = 0
    for key, d in dec.items():
        v = rec_ref[key].reshape(d.shape)
        differ = (v > 0) != d
        scale = float(v.abs().max())
        worst_v = float(v[differ].abs().max()) if bool(differ.any()) else 0.0
        assert worst_v <= tie_tol * scale, (key, worst_v, scale)
        assert int(differ.sum()) <= 10 * tie_tol * d.numel(), (key, int(differ.sum()))
        total += int(differ.sum())
    return total


@functools.lru_cache(maxsize=None)
def module_reference(config, gkey, training=True):
    """The float64 reference of a module case with its own decisions, computed once: (results, recorded ReLU pre-activations)."""
    rec = {}
    return module_eval(module_case(config, gkey, training), torch.float64, rec=rec), rec


def module_refs(case, dec):
    """The reference tensor of every judged tensor of a module case: out from the unconditioned float64 reference, the gradients
    from the float64 backward with the ReLU decisions `dec` of the side under test (which must differ from the reference's own only
    on near-ties).  -> ({tensor: reference}, number of decisions that differ, the conditioned results)."""
    free, rec = module_reference(case['config'], case['gkey'], case['training'])
    if not case['training']:
        return {'out': free['out']}, 0, free
    n_diff = check_near_ties(dec, rec)
    cond = free if n_diff == 0 else module_eval(case, torch.float64, dec=dec)
    return {k: (free if k == 'out' else cond)[k] for k in compared(case, cond)}, n_diff, cond


# (config, graph key, training) of every module case; tests/test_gpu_ecc_edges.py adds the launch form
MODULE_CASES = (
    [('matrix', g, True) for g in (3, 5, 200, 1008, 1024, 1025, 2049, 'scenes')] +
    [('vector', g, True) for g in (5, 200, 1008, 1024, 1025, 2049, 'scenes')] +
    [('plain', g, True) for g in (200, 1008, 1025, 2049)] +
    [('lstm', g, True) for g in (200, 1025)] +
    [('matrix', 200, False), ('matrix', 1025, False), ('vector', 1025, False)])

OP_CASES = ([(g, s, sc, False) for g in (5, 200) for s in OP_SHAPES for sc in OP_SCALES] +
            [('scenes', s, 1.0, False) for s in ('32x32 matrix', '32 vector')] + [(200, '10x15 matrix', 1.0, True)])
