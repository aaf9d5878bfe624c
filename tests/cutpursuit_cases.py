"""Inputs of the cut-pursuit tests (host and device): graphs with costs for the min cut, scenes for the partition solver.
Parallel-edge multiplicity stays <= 4 so that the summed capacities fit scipy's int32."""
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
