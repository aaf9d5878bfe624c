"""Named cases of the supervised loader's neighbourhood sub-sampling, shared by tests/test_spg_sample_cases.py (CPU: the numpy
restatement against the host path, and every case's claimed property) and tests/test_gpu_spg_sample.py (ops.sample_spg against
the host path).  The yardstick is `host_sample`: step 1 of learning/spg.py: loader, verbatim, on a SuperpointGraph --
permute_vertices / random_neighborhoods / k_big_enough, which tests/test_dropin.py pins to the imported reference.

A case = dict(n, edges i64 [E, 2], feats f32 [E, F], sizes i64 [n], nneigh, order, hardcutoff, minpts, seed) plus `why` (the
property that makes it a case) and `holds(ctx)` (that property, checked on ctx = dict(case, perm, centres, host, restate)).
Where a case needs particular centres, its seed is SEARCHED (seed_where) so that the host path's own random.sample draws them."""
import random

import numpy as np

F = 13
MINPTS = 40


def draw(case):
    """(perm, centres) as `loader` draws them under random.seed(case['seed']): the shuffle first, then the centres."""
    random.seed(case['seed'])
    n, perm, centres = case['n'], None, None
    if 0 < case['hardcutoff'] < n:
        perm = list(range(n))
        random.shuffle(perm)
    if 0 < case['nneigh'] < n:
        centres = random.sample(range(n), k=case['nneigh'])
    return perm, centres


def host_sample(case):
    """Step 1 of learning/spg.py: loader on the host -> dict(vids, edges, kept, feats, degs) of the sample."""
    from superpoint_graph_amd.learning import spg
    n, E = case['n'], len(case['edges'])
    G = spg.SuperpointGraph(n, case['edges'], True, {'f': list(case['feats']), 'id': list(range(E))},
                            {'v': list(range(n)), 's': list(case['sizes'])})
    random.seed(case['seed'])
    if 0 < case['hardcutoff'] < G.vcount():
        perm = list(range(G.vcount()))
        random.shuffle(perm)
        G = G.permute_vertices(perm)
    if 0 < case['nneigh'] < G.vcount():
        G = spg.random_neighborhoods(G, case['nneigh'], case['order'])
    if 0 < case['hardcutoff'] < G.vcount():
        G = spg.k_big_enough(G, case['minpts'], case['hardcutoff'])
    feats = np.asarray(G._eattrs['f'], dtype=np.float32).reshape(G.ecount(), F)
    return dict(vids=np.array(G.vs['v'], dtype=np.int64), edges=np.asarray(G._edges, dtype=np.int64).reshape(-1, 2),
                kept=np.array(G._eattrs['id'], dtype=np.int64), feats=feats, degs=np.array(G.indegree(), dtype=np.int64))


def restate(case, **override):
    import spg_sample_restatement as R
    c = dict(case, **override)
    perm, centres = draw(c)
    return R.sample(c['n'], c['edges'], c['sizes'], perm, centres, c['order'], c['minpts'], c['hardcutoff'])


def seed_where(case, pred, tries=20000):
    """The first seed under which the loader's own draws satisfy pred(perm, centres)."""
    for seed in range(tries):
        case['seed'] = seed
        if pred(*draw(case)):
            return case
    raise AssertionError('no seed found for ' + case['why'])


def _case(why, n, edges, nneigh, order, hardcutoff, sizes=None, minpts=MINPTS, seed=0, holds=None):
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    rs = np.random.RandomState(len(edges) * 7 + n)
    feats = rs.standard_normal((len(edges), F)).astype(np.float32)
    sizes = rs.randint(minpts - 3, minpts + 4, n).astype(np.int64) if sizes is None else np.asarray(sizes, dtype=np.int64)     # around minpts
    return dict(why=why, n=n, edges=edges, feats=feats, sizes=sizes, nneigh=nneigh, order=order, hardcutoff=hardcutoff, minpts=minpts,
                seed=seed, holds=holds or (lambda ctx: True))


def _random_edges(n, E, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, n, E), rs.randint(0, n, E)], 1)      # self-loops and repeated edges included


def _path(order):
    n = 40
    edges = [(i, i + 1) for i in range(n - 1)]                          # one direction only: the search ignores it
    reach = min(order, n - 1) + 1

    def holds(ctx):
        ok = ctx['centres'] == [0] and ctx['perm'] is None and list(ctx['host']['vids']) == list(range(reach))
        if order == 50:     # exhausted: no member is gained between order 49 and 50, and 38 is not enough
            ok = ok and restate(ctx['case'], order=49)['member'].sum() == n == restate(ctx['case'], order=50)['member'].sum()
            ok = ok and restate(ctx['case'], order=38)['member'].sum() == n - 1
        return ok
    c = _case(f'path of 40, the centre at one end, order {order}' + (' (the search exhausts)' if order == 50 else ''), n, edges, 1, order, 0,
              holds=holds)
    return seed_where(c, lambda perm, centres: centres == [0])


def _hub():
    n = 301
    edges = [(0, i) for i in range(1, n)] + [(i, 0) for i in range(1, n)]      # 600 incidences at vertex 0: more than one workgroup
    return _case('a hub with 300 incident edges in both directions', n, edges, 1, 2, 0,
                 holds=lambda ctx: len(ctx['host']['vids']) == n and len(ctx['host']['kept']) == 600)


def _loops():
    edges = [(0, 1), (2, 2), (1, 3), (1, 3), (1, 3), (3, 4), (4, 5), (5, 0), (2, 1)]
    c = _case('a self-loop and a triple repeated edge', 6, edges, 2, 1, 0,
              holds=lambda ctx: ctx['host']['kept'].tolist() == [0, 1, 2, 3, 4, 8])
    return seed_where(c, lambda perm, centres: sorted(centres) == [1, 2])


def _two_components():
    n = 20
    edges = [(i, (i + 1) % 10) for i in range(10)] + [(10 + i, 10 + (i + 1) % 10) for i in range(10)]
    c = _case('two components, all centres in one', n, edges, 3, 50, 0,
              holds=lambda ctx: sorted(ctx['host']['vids'].tolist()) == list(range(10)))
    return seed_where(c, lambda perm, centres: max(centres) < 10)


def _isolated():
    n = 30
    edges = [(i, (i + 1) % 10) for i in range(10)] + [(3, 7), (7, 3)]
    c = _case('isolated vertices among the centres', n, edges, 5, 1, 0,
              holds=lambda ctx: any(v >= 10 for v in ctx['host']['vids']) and len(ctx['host']['kept']) > 0)
    return seed_where(c, lambda perm, centres: sum(v >= 10 for v in centres) >= 2 and sum(v < 10 for v in centres) >= 2)


def _no_edge():
    n = 12
    edges = [(2 * i, 2 * i + 1) for i in range(6)] + [(2 * i + 1, 2 * i) for i in range(6)]
    c = _case('a sample that keeps vertices but no edge', n, edges, 2, 0, 0,
              holds=lambda ctx: len(ctx['host']['vids']) == 2 and len(ctx['host']['kept']) == 0)
    return seed_where(c, lambda perm, centres: centres[0] // 2 != centres[1] // 2)


def _members(ctx):
    """members of the case's own draws, before any cut"""
    import spg_sample_restatement as R
    c = ctx['case']
    return int(R.sample(c['n'], c['edges'], c['sizes'], ctx['perm'], ctx['centres'], c['order'])['member'].sum())


def _s3dis():
    from superpoint_graph_amd import synth
    sc = synth.scene(seed=0, n_sp=1000, n_edges=5000, n_pts=8)
    n = int(sc['n_sp'])
    sizes = np.clip(np.round(np.random.RandomState(5).lognormal(np.log(60.0), 1.0, n)), 1, 5000).astype(np.int64)
    c = _case('the S3DIS shape: 1000 / 5000, 100 centres, order 3, cut 512', n, sc['edges'], 100, 3, 512, sizes=sizes,
              holds=lambda ctx: ctx['perm'] is not None and len(ctx['centres']) == 100 and 0 < len(ctx['host']['kept']) < 5000)
    c['feats'] = np.ascontiguousarray(sc['edge_feats'], dtype=np.float32)
    return c


def build():
    n60 = 60
    e60 = _random_edges(n60, 180, 11)
    cases = {
        'n1_e0': _case('one vertex, no edge: the sample is dropped', 1, np.zeros((0, 2)), 100, 3, 512,
                       holds=lambda ctx: len(ctx['host']['vids']) == 1 and len(ctx['host']['kept']) == 0),
        'n2_one_edge': _case('two vertices, one edge', 2, [(1, 0)], 1, 1, 1, sizes=[MINPTS, MINPTS - 1],
                             holds=lambda ctx: ctx['perm'] is not None and ctx['centres'] is not None),
        'path_order0': _path(0), 'path_order1': _path(1), 'path_order3': _path(3), 'path_order50': _path(50),
        'hub300': _hub(), 'selfloop_triple': _loops(), 'two_components': _two_components(), 'isolated_centres': _isolated(),
        'nneigh_ge_n': _case('nneigh >= n: no centres, every vertex is a member', n60, e60, n60, 3, 20,
                             holds=lambda ctx: ctx['centres'] is None and ctx['perm'] is not None and len(ctx['host']['vids']) < n60),
        'hardcutoff_ge_n': _case('hardcutoff >= n: no perm, no cut', n60, e60, 4, 1, n60 + 5,
                                 holds=lambda ctx: ctx['perm'] is None and len(ctx['host']['vids']) == _members(ctx) < n60),
        'hardcutoff_above_members': _case('hardcutoff between the member count and n: perm applied, the cut keeps all', n60, e60, 2, 1, n60 - 1,
                                          holds=lambda ctx: ctx['perm'] is not None and len(ctx['host']['vids']) == _members(ctx) < n60 - 1),
        'hardcutoff_1': _case('hardcutoff = 1', n60, e60, 6, 2, 1,
                              holds=lambda ctx: 0 < len(ctx['host']['vids']) < _members(ctx)
                              and (ctx['case']['sizes'][ctx['host']['vids']] >= MINPTS).sum() == 1),
        's_eq_minpts': _case('s == minpts exactly: every member counts as big', n60, e60, 10, 2, 7, sizes=np.full(n60, MINPTS),
                             holds=lambda ctx: len(ctx['host']['vids']) == 7 < _members(ctx)),
        'all_small': _case('every s < minpts: the cut never bites', n60, e60, 10, 2, 1, sizes=np.full(n60, MINPTS - 1),
                           holds=lambda ctx: len(ctx['host']['vids']) == _members(ctx) > 1),
        'no_edge_kept': _no_edge(),
        's3dis': _s3dis(),
    }
    for n in (255, 256, 257, 1025):       # block boundaries of the vertex and the edge launches (workgroups of 256)
        cases[f'blocks_{n}'] = _case(f'n = {n}, E = 3n: a block boundary', n, _random_edges(n, 3 * n, n), n // 3 + 1, 1, n // 2 + 1, seed=n,
                                     holds=lambda ctx: 0 < len(ctx['host']['vids']) < ctx['case']['n'] and len(ctx['host']['kept']) > 0)
    return cases


_CASES = None


def cases():
    """The cases with their host results, built once and shared: name -> (case, perm, centres, host result)."""
    global _CASES
    if _CASES is None:
        _CASES = {}
        for name, c in build().items():
            perm, centres = draw(c)
            _CASES[name] = (c, perm, centres, host_sample(c))
    return _CASES


NAMES = ['n1_e0', 'n2_one_edge', 'path_order0', 'path_order1', 'path_order3', 'path_order50', 'hub300', 'selfloop_triple', 'two_components',
         'isolated_centres', 'nneigh_ge_n', 'hardcutoff_ge_n', 'hardcutoff_above_members', 'hardcutoff_1', 's_eq_minpts', 'all_small',
         'no_edge_kept', 's3dis', 'blocks_255', 'blocks_256', 'blocks_257', 'blocks_1025']
