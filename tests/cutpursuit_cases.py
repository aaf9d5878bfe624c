"""Inputs of the cut-pursuit tests (host and device): graphs with costs for the min cut, scenes for the partition solver.
Parallel-edge multiplicity stays <= 4 so that the summed capacities fit scipy's int32.

Below the scenes: the references that share no code with the kernels or the restatement (test_cutpursuit_cases.py,
test_gpu_cutpursuit_edges.py): an exhaustive min-cut oracle with its graphs, closed-form min-cut cases at the constants of the
host loop, shapes / keys / values and plain references of the three per-component entry points, power-of-two scalings of a
scene, and edge scenes of the solver."""
import functools

import numpy as np

CAP_MAX = (1 << 28) - 1


def _random_graph(rng, n, E, cap_hi=1000, cost_hi=2000):
    src = rng.integers(0, n, E)
    tgt = rng.integers(0, n, E)
    cap = rng.integers(0, cap_hi, E)
    u = rng.integers(-cost_hi, cost_hi, n)
    return dict(n=n, src=src, tgt=tgt, cap=cap, cost0=np.maximum(u, 0), cost1=np.maximum(-u, 0))


def grid_edges(h, w):
    idx = np.arange(h * w).reshape(h, w)
    src = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    tgt = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return src, tgt


def mincut_cases():
    rng = np.random.default_rng(20)
    cases = {}
    cases['n1'] = dict(n=1, src=np.zeros(0, np.int64), tgt=np.zeros(0, np.int64), cap=np.zeros(0, np.int64),
                       cost0=np.array([3]), cost1=np.array([5]))
    cases['n1_loop'] = dict(n=1, src=np.array([0]), tgt=np.array([0]), cap=np.array([7]), cost0=np.array([5]), cost1=np.array([3]))
    cases['n2'] = dict(n=2, src=np.array([0]), tgt=np.array([1]), cap=np.array([4]), cost0=np.array([0, 9]), cost1=np.array([6, 0]))
    for n in (63, 64, 65, 257):
        cases[f'random{n}'] = _random_graph(rng, n, 3 * n)
    # the only source and the only sink at opposite ends of a path: one pulse per hop
    n = 300
    c0, c1 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    c1[0], c0[n - 1] = 50, 70
    cases['path300'] = dict(n=n, src=np.arange(n - 1), tgt=np.arange(1, n), cap=rng.integers(40, 90, n - 1), cost0=c0, cost1=c1)
    src, tgt = grid_edges(16, 16)
    u = rng.integers(-300, 300, 256)
    cases['grid16'] = dict(n=256, src=src, tgt=tgt, cap=rng.integers(0, 120, len(src)), cost0=np.maximum(u, 0), cost1=np.maximum(-u, 0))
    # a hub of degree 100 that has to spread its excess over its spokes
    n = 101
    c0, c1 = rng.integers(0, 40, n), np.zeros(n, np.int64)
    c0[0], c1[0] = 0, 2500
    cases['hub100'] = dict(n=n, src=np.zeros(100, np.int64), tgt=np.arange(1, 101), cap=rng.integers(0, 50, 100), cost0=c0, cost1=c1)
    # self-loops, parallel edges (multiplicity 4) and zero capacities
    g = _random_graph(rng, 40, 60)
    loops = rng.integers(0, 40, 10)
    src = np.concatenate([g['src'], g['src'][:20], g['tgt'][:20], g['src'][:20], loops])
    tgt = np.concatenate([g['tgt'], g['tgt'][:20], g['src'][:20], g['tgt'][:20], loops])
    cap = rng.integers(0, 1000, len(src))
    cap[::5] = 0
    cases['loops_parallel_zero'] = dict(g, src=src, tgt=tgt, cap=cap)
    g = _random_graph(rng, 90, 200)
    both0 = rng.random(90) < 0.6
    cases['both_costs_zero'] = dict(g, cost0=np.where(both0, 0, g['cost0']), cost1=np.where(both0, 0, g['cost1']))
    g = _random_graph(rng, 70, 150)
    cases['all_cost0'] = dict(g, cost0=g['cost0'] + g['cost1'], cost1=np.zeros(70, np.int64))
    cases['all_cost1'] = dict(g, cost1=g['cost0'] + g['cost1'], cost0=np.zeros(70, np.int64))
    # several disconnected parts, one of them without any cost
    parts, off, S, T, C = [], 0, [], [], []
    for n_p in (30, 1, 45, 20):
        gp = _random_graph(rng, n_p, 2 * n_p)
        S.append(gp['src'] + off); T.append(gp['tgt'] + off); C.append(gp['cap'])
        parts.append(gp); off += n_p
    c0 = np.concatenate([p['cost0'] for p in parts]); c1 = np.concatenate([p['cost1'] for p in parts])
    c0[-20:], c1[-20:] = 0, 0
    cases['disconnected'] = dict(n=off, src=np.concatenate(S), tgt=np.concatenate(T), cap=np.concatenate(C), cost0=c0, cost1=c1)
    g = _random_graph(rng, 50, 120, cap_hi=CAP_MAX + 1, cost_hi=CAP_MAX + 1)
    g['cap'][:40] = CAP_MAX
    g['cost0'][:10], g['cost1'][:10] = CAP_MAX, 0
    g['cost1'][10:20], g['cost0'][10:20] = CAP_MAX, 0
    cases['cap_max'] = g
    return {k: {a: (np.asarray(v, np.int64) if a != 'n' else v) for a, v in c.items()} for k, c in cases.items()}


# ------------------------------------------------------------------------------------------------------------------
def planted_grid(side, D, noise, seed, split=None):
    """side x side 4-connected grid, four planted rectangles with well separated values in every dimension"""
    rng = np.random.default_rng(seed)
    a, b = split or (side * 2 // 5, side * 3 // 5)
    r, c = np.divmod(np.arange(side * side), side)
    planted = (r >= a).astype(np.int64) * 2 + (c >= b)
    level = np.stack([rng.permutation(4) for _ in range(D)], 1).astype(np.float64)        # [4, D]
    obs = (level[planted] + noise * rng.standard_normal((side * side, D))).astype(np.float32)
    src, tgt = grid_edges(side, side)
    return obs, src, tgt, planted


def solver_cases():
    """name -> dict(obs, src, tgt, w, m, planted or None, kwargs of cut_pursuit)"""
    cases = {}
    for D, noise, lam in ((1, 0.05, 0.2), (2, 0.1, 0.3), (7, 0.1, 0.3), (32, 0.05, 0.3)):
        obs, src, tgt, planted = planted_grid(20, D, noise, seed=D)
        cases[f'planted_D{D}'] = dict(obs=obs, src=src, tgt=tgt, w=np.ones(len(src), np.float32), m=None, planted=planted,
                                      kw=dict(reg_strength=lam))
    obs, src, tgt, planted = planted_grid(24, 3, 0.08, seed=11, split=(7, 15))
    rng = np.random.default_rng(5)
    w = rng.uniform(0.5, 1.5, len(src)).astype(np.float32)
    m = rng.uniform(0.5, 2.0, len(obs)).astype(np.float32)
    cases['planted_weighted'] = dict(obs=obs, src=src, tgt=tgt, w=w, m=m, planted=planted, kw=dict(reg_strength=0.2))
    # over-segmentation (small regularisation) with and without the merge of small components, and a decaying regularisation
    cases['overseg'] = dict(obs=obs, src=src, tgt=tgt, w=w, m=m, planted=None, kw=dict(reg_strength=0.002))
    cases['overseg_cutoff10'] = dict(obs=obs, src=src, tgt=tgt, w=w, m=m, planted=None, kw=dict(reg_strength=0.002, cutoff=10))
    cases['decay07'] = dict(obs=obs, src=src, tgt=tgt, w=w, m=m, planted=None, kw=dict(reg_strength=0.3, weight_decay=0.7))
    cases['decay07_cutoff10'] = dict(obs=obs, src=src, tgt=tgt, w=w, m=m, planted=None,
                                     kw=dict(reg_strength=0.02, weight_decay=0.7, cutoff=10))
    # the inpainting shape: labels as observations, most vertices without weight
    obs1, src1, tgt1, planted1 = planted_grid(20, 1, 0.0, seed=3)
    known = (rng.random(len(obs1)) < 0.3).astype(np.float32)
    cases['inpainting'] = dict(obs=obs1, src=src1, tgt=tgt1, w=np.ones(len(src1), np.float32), m=known, planted=None,
                               kw=dict(reg_strength=0.01))
    dup = np.tile(np.float32([[0.25, -3.0, 7.5]]), (50, 1))
    cases['duplicates'] = dict(obs=dup, src=np.arange(49), tgt=np.arange(1, 50), w=np.ones(49, np.float32), m=None, planted=None,
                               kw=dict(reg_strength=0.1))
    cases['n1'] = dict(obs=np.float32([[1.5, 2.5]]), src=np.zeros(0, np.int64), tgt=np.zeros(0, np.int64), w=np.zeros(0, np.float32),
                       m=None, planted=None, kw=dict(reg_strength=0.1))
    return cases


# ------------------------------------------------------------------------------------------------------------------
# A. the exhaustive min-cut oracle and its graphs
# ------------------------------------------------------------------------------------------------------------------
ORACLE_MAX_N = 12


def _case(n, src, tgt, cap, cost0, cost1, **more):
    i64 = lambda a: np.asarray(a, np.int64).reshape(-1)
    return dict(n=int(n), src=i64(src), tgt=i64(tgt), cap=i64(cap), cost0=i64(cost0), cost1=i64(cost1), **more)


def exhaustive_min_cut(n, src, tgt, cap, cost0, cost1):
    """-> (label uint8 [n], value, number of minimisers): all 2^n labelings, energy sum cost_label(v) + sum cap_e [l_u != l_v] in
    int64, the elementwise minimum over the minimisers.  The minimisers of a submodular energy are closed under intersection, so
    that minimum is a minimiser itself and the only one with the fewest ones: asserted."""
    assert 1 <= n <= ORACLE_MAX_N
    src, tgt, cap, cost0, cost1 = (np.asarray(a, np.int64) for a in (src, tgt, cap, cost0, cost1))
    shifts = np.arange(n, dtype=np.int64)
    bits = (np.arange(1 << n, dtype=np.int64)[:, None] >> shifts) & 1                          # [2^n, n], row = its own code
    energy = np.where(bits == 1, cost1, cost0).sum(1) + ((bits[:, src] != bits[:, tgt]) * cap).sum(1)
    best = energy.min()
    minimisers = bits[energy == best]
    label = minimisers.min(0)
    assert energy[int((label << shifts).sum())] == best
    assert (minimisers.sum(1) == label.sum()).sum() == 1
    return label.astype(np.uint8), int(best), len(minimisers)


ORACLE_GRAPHS = 240
ORACLE_ONE_BY_ONE = (0, 1, 2, 3, 4) + tuple(range(5, ORACLE_GRAPHS, 16))       # 20 graphs; 0: n = 1, E = 0; 2, 4: n > 1, E = 0


@functools.lru_cache(maxsize=None)
def oracle_graphs():
    """ORACLE_GRAPHS graphs with n in 1..12 and E in 0..3n, self-loops and parallel edges as they fall, values below 2, 4 or 1000
    (the small ranges force ties), a third of them with both costs positive on every vertex; each with the oracle's 'label',
    'value' and 'minimisers'.  At least a quarter have more than one minimiser: asserted here, on the oracle alone."""
    rng = np.random.default_rng(411)
    fixed = ((1, 0), (1, 2), (5, 0), (12, 36), (12, 0))
    graphs = []
    for i in range(ORACLE_GRAPHS):
        n, E = fixed[i] if i < len(fixed) else (int(rng.integers(1, 13)), None)
        E = int(rng.integers(0, 3 * n + 1)) if E is None else E
        hi = (2, 4, 1000)[i % 3]
        if (i // 3) % 3 == 0:
            cost0, cost1 = rng.integers(1, hi, n), rng.integers(1, hi, n)
        else:
            u = rng.integers(1 - hi, hi, n)
            cost0, cost1 = np.maximum(u, 0), np.maximum(-u, 0)
        g = _case(n, rng.integers(0, n, E), rng.integers(0, n, E), rng.integers(0, hi, E), cost0, cost1)
        g['label'], g['value'], g['minimisers'] = exhaustive_min_cut(**g)
        graphs.append(g)
    assert 4 * sum(g['minimisers'] > 1 for g in graphs) >= len(graphs)
    assert 3 * sum(bool(np.all((g['cost0'] > 0) & (g['cost1'] > 0))) for g in graphs) >= len(graphs)
    return tuple(graphs)


def disjoint_union(graphs):
    """one graph of all: vertex offsets, edges concatenated; 'label' / 'value' where the parts have them"""
    off = np.cumsum([0] + [g['n'] for g in graphs])
    cat = lambda k, add=False: np.concatenate([g[k] + (o if add else 0) for g, o in zip(graphs, off)])
    u = _case(off[-1], cat('src', True), cat('tgt', True), cat('cap'), cat('cost0'), cat('cost1'), offsets=off)
    if all('label' in g for g in graphs):
        u['label'], u['value'] = np.concatenate([g['label'] for g in graphs]), sum(g['value'] for g in graphs)
    return u


# ------------------------------------------------------------------------------------------------------------------
# B. min-cut cases with closed forms, at the constants of the host loop (16 pulses, 16 levels, blocks of 256)
# ------------------------------------------------------------------------------------------------------------------
PATH_NS = (2, 15, 16, 17, 18, 31, 32, 33, 34)
PATH_FAMILIES = ('through', 'bottleneck', 'sink_limited')


def path_case(n, family):
    """A path 0 - 1 - ... - n-1, caps 7, the only source at vertex 0, the only sink at vertex n - 1.
    through:       source 5, sink 9: the source arc is the cut, every vertex still reaches the sink: all 1, value 5, one pulse per
                   hop ('pulses' = n)
    bottleneck:    source 9, sink 12, one cap of 3 in the middle: 1 exactly on the sink side of it, value 3
    sink_limited:  source 9, sink 4: the sink arc is the cut, nobody reaches the sink: all 0, value 4"""
    cost0, cost1, cap = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n - 1, 7, np.int64)
    more = {}
    if family == 'through':
        cost1[0], cost0[n - 1] = 5, 9
        label, value, more = np.ones(n, np.uint8), 5, dict(pulses=n)
    elif family == 'bottleneck':
        cost1[0], cost0[n - 1] = 9, 12
        b = (n - 2) // 2
        cap[b] = 3
        label, value = (np.arange(n) > b).astype(np.uint8), 3
    else:
        assert family == 'sink_limited'
        cost1[0], cost0[n - 1] = 9, 4
        label, value = np.zeros(n, np.uint8), 4
    return _case(n, np.arange(n - 1), np.arange(1, n), cap, cost0, cost1, label=label, value=value, **more)


EDGELESS_NS = (255, 256, 257, 512)


def edgeless_case(n):
    """n > 1 vertices, no edge: label = cost1 < cost0, a tie gives 0; ties, vertices with both costs 0 and values at the limit"""
    rng = np.random.default_rng(n)
    cost0, cost1 = rng.integers(0, 6, n), rng.integers(0, 6, n)
    cost0[::7] = CAP_MAX
    cost1[3::7] = CAP_MAX
    cost0[5::14], cost1[5::14] = CAP_MAX, CAP_MAX
    assert ((cost0 == cost1) & (cost0 > 0)).any() and ((cost0 == 0) & (cost1 == 0)).any()
    none = np.zeros(0, np.int64)
    return _case(n, none, none, none, cost0, cost1, label=(cost1 < cost0).astype(np.uint8), value=int(np.minimum(cost0, cost1).sum()))


STAR_ARMS = 17
STAR_M = CAP_MAX


def double_star(c):
    """Vertex 0 is the centre; STAR_ARMS sources (cost1 = M, an edge of cap M to the centre) and as many sinks (cost0 = M, an edge of
    cap c from the centre).  After the first pulse the centre holds 17 M > 2^32.  c = M - 1: the sink edges are the cut, value
    17 (M - 1), only the sinks are 1; c = M: everything is saturated, nobody reaches the sink, all 0, value 17 M."""
    a, M = STAR_ARMS, STAR_M
    assert a * M > 1 << 31 and c in (M - 1, M)
    n = 1 + 2 * a
    cost0, cost1 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    cost1[1:1 + a], cost0[1 + a:] = M, M
    src = np.concatenate([np.arange(1, 1 + a), np.zeros(a, np.int64)])
    tgt = np.concatenate([np.zeros(a, np.int64), np.arange(1 + a, n)])
    cap = np.concatenate([np.full(a, M), np.full(a, c)])
    label = np.zeros(n, np.uint8)
    if c < M:
        label[1 + a:] = 1
    return _case(n, src, tgt, cap, cost0, cost1, label=label, value=a * c)


def no_source_cases():
    """No vertex has cost1 > 0, so nothing is ever active and max_pulses = 0 suffices.  'no_cost': no cost at all: all 0.
    'cost0_only': label 1 is free, and the minimiser with the fewest ones is 1 exactly where a vertex with cost0 > 0 can be
    reached over edges of positive cap (a plain fixed point here), value 0."""
    rng = np.random.default_rng(30)
    n, E = 40, 50
    src, tgt, cap = rng.integers(0, n, E), rng.integers(0, n, E), rng.integers(0, 4, E)
    zero = np.zeros(n, np.int64)
    cost0 = np.where(rng.random(n) < 0.15, rng.integers(1, 9, n), 0)
    label = cost0 > 0
    for _ in range(n):
        for e in np.nonzero(cap > 0)[0]:
            label[src[e]] = label[tgt[e]] = label[src[e]] or label[tgt[e]]
    assert 0 < label.sum() < n
    return {'no_cost': _case(n, src, tgt, cap, zero, zero, label=np.zeros(n, np.uint8), value=0),
            'cost0_only': _case(n, src, tgt, cap, cost0, zero, label=label.astype(np.uint8), value=0)}


# ------------------------------------------------------------------------------------------------------------------
# C. the per-component entry points: shapes, keys, values, plain references
# ------------------------------------------------------------------------------------------------------------------
CP_NS, CP_DS = (1, 63, 64, 65, 255, 256, 257, 1000), (1, 3, 32)
CP_KS = (1, 2, 7, 'n')
CP_KEY_PATTERNS = ('one_key', 'holes', 'wave_runs', 'shifted_runs', 'random', 'all_minus1', 'out_of_range')
# (n, D, K, key pattern); K = 0 stands for K = n
CP_SHAPES = (
    (1, 1, 1, 'one_key'), (1, 3, 1, 'all_minus1'), (1, 32, 0, 'out_of_range'),
    (63, 3, 2, 'holes'), (63, 1, 7, 'random'),
    (64, 32, 1, 'one_key'), (64, 3, 7, 'holes'), (64, 1, 0, 'random'),
    (65, 3, 2, 'wave_runs'), (65, 32, 7, 'shifted_runs'), (65, 1, 0, 'out_of_range'),
    (255, 3, 2, 'shifted_runs'), (255, 1, 7, 'wave_runs'), (255, 32, 0, 'random'),
    (256, 1, 1, 'one_key'), (256, 3, 2, 'wave_runs'), (256, 32, 7, 'out_of_range'), (256, 3, 0, 'shifted_runs'),
    (257, 3, 1, 'holes'), (257, 1, 2, 'random'), (257, 32, 7, 'wave_runs'), (257, 3, 0, 'all_minus1'),
    (1000, 3, 7, 'shifted_runs'), (1000, 32, 2, 'holes'), (1000, 1, 0, 'wave_runs'), (1000, 3, 7, 'out_of_range'),
    (1000, 32, 0, 'random'),
)
CP_VALUE_PATTERNS = ('random', 'cancel', 'negative')
CP_FAR_PATTERNS = ('ties', 'zero_weight_max', 'weightless_key', 'all_zero_dist', 'span')
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def cp_shape_id(shape):
    n, D, K, pattern = shape
    return f'n{n}_D{D}_K{K or "n"}_{pattern}'


def cp_keys(shape, rng):
    """-> (key int32 [n], K)
    one_key:       all vertices share key K - 1 (every other row has no member)
    holes:         key K - 1 with -1 holes, lane 0 of the first wave among the holes
    wave_runs:     runs of 64 aligned to the wave, key = wave mod K
    shifted_runs:  the same runs shifted by one vertex, so that every wave is mixed
    random, all_minus1
    out_of_range:  random keys with values >= K and < -1 mixed in (the int32 extremes among them), which must be ignored"""
    n, _, K, pattern = shape
    K = K or n
    v = np.arange(n)
    if pattern == 'one_key':
        key = np.full(n, K - 1)
    elif pattern == 'holes':
        key = np.where(rng.random(n) < 0.4, -1, K - 1)
        key[0] = -1
    elif pattern == 'wave_runs':
        key = (v // 64) % K
    elif pattern == 'shifted_runs':
        key = ((v + 1) // 64) % K
    elif pattern == 'random':
        key = rng.integers(0, K, n)
    elif pattern == 'all_minus1':
        key = np.full(n, -1)
    else:
        assert pattern == 'out_of_range'
        key, r = rng.integers(0, K, n), rng.random(n)
        key = np.where(r < 0.2, K + rng.integers(0, 5, n), np.where(r < 0.4, -2 - rng.integers(0, 5, n), np.where(r < 0.5, -1, key)))
        key[:4] = np.array([K, -2, I32_MAX, I32_MIN])[:n]
    return key.astype(np.int32), K


def cp_values(pattern, n, D, rng):
    """-> (mq int64 [n] in [0, 2^10], q int64 [n, D] in +-2^20)
    random:    a fifth of the weights 0, the whole second wave without weight, a tenth of q zero
    cancel:    vertices 2i and 2i + 1 carry the same weight and opposite q: exactly 0 inside a wave, and inside a key that holds both
    negative:  q <= 0 throughout: a negative total"""
    half = (n + 1) // 2
    if pattern == 'random':
        mq = rng.integers(0, 1025, n)
        mq[rng.random(n) < 0.2] = 0
        mq[64:128] = 0
        q = rng.integers(-(1 << 20), (1 << 20) + 1, (n, D))
        q[rng.random((n, D)) < 0.1] = 0
    elif pattern == 'cancel':
        mq = np.repeat(rng.integers(1, 1025, half), 2)[:n]
        q = np.repeat(rng.integers(-(1 << 20), (1 << 20) + 1, (half, D)), 2, axis=0)[:n]
        q[1::2] = -q[1::2]
        if n % 2:
            q[n - 1] = 0
    else:
        assert pattern == 'negative'
        mq = rng.integers(1, 1025, n)
        q = -rng.integers(0, (1 << 20) + 1, (n, D))
    return mq.astype(np.int64), q.astype(np.int64)


def cp_sums_ref(key, mq, q, K):
    """W [K], S [K, D] with Python integers (-> int64, asserted to fit): the vertices with 0 <= key < K"""
    n, D = q.shape
    W, S = [0] * K, [[0] * D for _ in range(K)]
    for v in range(n):
        k, m = int(key[v]), int(mq[v])
        if 0 <= k < K and m:
            W[k] += m
            row = S[k]
            for d, x in enumerate(q[v].tolist()):
                row[d] += m * x
    assert all(-(1 << 63) <= x < 1 << 63 for row in S for x in row)
    return np.array(W, np.int64), np.array(S, np.int64).reshape(K, D)


def cp_centres(key, mq, q, K, rng):
    """C f64 [K, D], non-integer: the quotient of two int64 sums, as the solver makes it, where a key has weight; elsewhere a
    quotient of magnitude up to 2^21"""
    W, S = cp_sums_ref(key, mq, q, K)
    C = rng.integers(-(1 << 40), 1 << 40, S.shape).astype(np.float64) / rng.integers(1, 1 << 19, (K, 1)).astype(np.float64)
    has = W > 0
    C[has] = S[has].astype(np.float64) / W[has].astype(np.float64)[:, None]
    return C


def cp_dist_ref(q, key, C):
    """float64, dimension by dimension: acc = acc + (q - C) * (q - C), each operation rounded on its own; +0.0 outside [0, K)"""
    n, D = q.shape
    inside = (key >= 0) & (key < C.shape[0])
    row = np.where(inside, key, 0)
    acc = np.zeros(n, np.float64)
    for d in range(D):
        diff = q[:, d].astype(np.float64) - C[row, d]
        sq = diff * diff
        acc = acc + sq
    return np.where(inside, acc, 0.0)


def cp_far_inputs(pattern, key, K, rng):
    """-> (dist f64 [n] >= +0.0, mq int64 [n])
    ties:             a few values, duplicated many times, two of them one ulp apart
    zero_weight_max:  the strict maximum of every key sits on a vertex without weight, which is skipped
    weightless_key:   every member of the lowest key present has mq = 0 (idx = n, best = 0.0)
    all_zero_dist:    all distances 0.0: the first positive-weight member
    span:             0.0, 5e-324, 1.0 and 1e300"""
    n = len(key)
    inside = (key >= 0) & (key < K)
    mq = rng.integers(1, 1025, n)
    mq[rng.random(n) < 0.2] = 0
    if pattern == 'ties':
        dist = rng.choice(np.array([0.0, 1.0, 2.5, np.nextafter(2.5, 3.0)]), n)
    elif pattern == 'zero_weight_max':
        dist = np.floor(rng.random(n) * 1000.0) / 8.0
        for k in np.unique(key[inside]):
            members = np.nonzero(key == k)[0]
            v = members[len(members) // 2]
            dist[v], mq[v] = 1e6, 0
    elif pattern == 'weightless_key':
        dist = rng.choice(np.array([0.0, 0.5, 3.0]), n)
        if inside.any():
            mq[key == key[inside].min()] = 0
    elif pattern == 'all_zero_dist':
        dist = np.zeros(n)
    else:
        assert pattern == 'span'
        dist = rng.choice(np.array([0.0, 5e-324, 1.0, 1e300]), n)
    return dist.astype(np.float64), mq.astype(np.int64)


def cp_farthest_ref(dist, key, mq, K):
    """the definition: per key, among the members with mq > 0, the largest dist and the lowest index that has it; (n, 0.0) if none"""
    n = len(dist)
    idx, best = [n] * K, [0.0] * K
    for v in range(n):
        k = int(key[v])
        if 0 <= k < K and mq[v] > 0 and (idx[k] == n or dist[v] > best[k]):
            idx[k], best[k] = v, float(dist[v])
    return np.array(idx, np.int64), np.array(best, np.float64)


# ------------------------------------------------------------------------------------------------------------------
# D. power-of-two scalings of a scene that the solver must follow exactly
# ------------------------------------------------------------------------------------------------------------------
SCALING_SCENES = ('planted_weighted', 'overseg_cutoff10', 'decay07_cutoff10', 'inpainting')
SCALINGS = ('obs_8', 'node_weight_4', 'edge_weight_quarter')


def scaled_scene(c, variant):
    """-> (scene, factor of the values, factor of every energy).  The quantisation is relative to the largest exponent, so each
    factor shifts only kf, km or the regularisation by a power of two: partition, pulses and merge rounds stay."""
    lam = c['kw']['reg_strength']
    if variant == 'obs_8':
        return dict(c, obs=c['obs'] * np.float32(8), kw=dict(c['kw'], reg_strength=lam * 64)), 8.0, 64.0
    if variant == 'node_weight_4':
        return dict(c, m=c['m'] * np.float32(4), kw=dict(c['kw'], reg_strength=lam * 4)), 1.0, 4.0
    assert variant == 'edge_weight_quarter'
    return dict(c, w=c['w'] * np.float32(0.25), kw=dict(c['kw'], reg_strength=lam * 4)), 1.0, 1.0


# ------------------------------------------------------------------------------------------------------------------
# E. solver scenes at the edges of its inputs and options
# ------------------------------------------------------------------------------------------------------------------
def edge_solver_cases():
    cases = {}
    rng = np.random.default_rng(130)
    # 130 vertices, the last ten isolated; self-loops, parallel edges, zero edge weights, zero node weights
    n, live = 130, 120
    src, tgt, loops = rng.integers(0, live, 300), rng.integers(0, live, 300), rng.integers(0, live, 12)
    src, tgt = np.concatenate([src, src[:40], tgt[40:80], loops]), np.concatenate([tgt, tgt[:40], src[40:80], loops])
    w = rng.uniform(0.2, 1.5, len(src)).astype(np.float32)
    w[::6] = 0
    m = rng.uniform(0.5, 2.0, n).astype(np.float32)
    m[::9] = 0
    obs = (rng.integers(0, 3, n)[:, None] + 0.1 * rng.standard_normal((n, 3))).astype(np.float32)
    cases['random130'] = dict(obs=obs, src=src, tgt=tgt, w=w, m=m, planted=None, kw=dict(reg_strength=0.05))
    cases['random130_cutoff5'] = dict(cases['random130'], kw=dict(reg_strength=0.05, cutoff=5))
    obs, src, tgt, planted = planted_grid(12, 3, 0.08, seed=12)
    n, E = len(obs), len(src)
    w = rng.uniform(0.25, 1.0, E).astype(np.float32)
    m = rng.uniform(0.5, 2.0, n).astype(np.float32)
    base = dict(obs=obs, src=src, tgt=tgt, w=w, m=m, planted=None, kw=dict(reg_strength=0.2))
    f32 = np.float32
    outlier = obs.copy()
    outlier[77, 1] = 1e30
    none = np.zeros(0, np.int64)
    cases['grid_obs_zero'] = dict(base, obs=np.zeros_like(obs))
    cases['grid_node_weight_zero'] = dict(base, m=np.zeros(n, f32))
    cases['grid_edge_weight_zero'] = dict(base, w=np.zeros(E, f32))
    cases['grid_reg_zero'] = dict(base, kw=dict(reg_strength=0.0))
    cases['grid_outlier_1e30'] = dict(base, obs=outlier)
    cases['grid_obs_1e-38'] = dict(base, obs=obs * f32(1e-38), kw=dict(reg_strength=1e-77))
    cases['grid_obs_5e37'] = dict(base, obs=obs * f32(5e37), kw=dict(reg_strength=1e74))
    cases['grid_edge_weight_3e38'] = dict(base, w=w * f32(3e38), kw=dict(reg_strength=1e-39))
    cases['grid_max_ite0'] = dict(base, kw=dict(reg_strength=0.2, max_ite=0))
    cases['grid_kmeans_ite0'] = dict(base, kw=dict(reg_strength=0.2, kmeans_ite=0))
    cases['grid_flow_steps1'] = dict(base, kw=dict(reg_strength=0.2, flow_steps=1))
    cases['grid_no_edges'] = dict(base, src=none, tgt=none, w=np.zeros(0, f32))
    for c in cases.values():
        assert all(np.isfinite(c[k]).all() for k in ('obs', 'w', 'm'))
    return cases
