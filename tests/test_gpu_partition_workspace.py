"""Every workspace-taking entry point of the partition units (spg_spgraph, spg_knn, spg_edgeloss, spg_parteval, spg_tiles,
spg_plane; spg_structure_frame and spg_parsed_stats by the same helper in tests/test_gpu_structure.py and tests/test_gpu_parsed.py)
through ctypes: a buffer of exactly spg_*_workspace_bytes bytes is enough and gives, bit for bit, what the ops wrapper
gives; with one byte less the call is refused before anything is written and the error names the size query.
Two sizes each: the smallest legal one, and one past a 256-thread block (n = 1 / 257, E = 1 / 300); the plane fit's smallest is
n = n_low = 3, and its larger one, 1300 low points, is past one workgroup of its trial pass (1024 points), with 1 and 100 trials."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (257, 300)]
i32, i64, u8, f32, f64 = torch.int32, torch.int64, torch.uint8, torch.float32, torch.float64


@pytest.fixture(scope='module')
def L():
    from superpoint_graph_amd._lib import lib
    return lib()


def P(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def fresh(*specs):
    """(count, dtype) ... -> output tensors filled with a byte pattern no kernel here produces by accident"""
    return [torch.full((count * torch.empty(0, dtype=dtype).element_size(),), 0xA5, dtype=u8, device='cuda').view(dtype) for count, dtype in specs]


def same(a, b):
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(u8), b.view(u8))


def exact_and_short(L, query, nbytes, make, call, expected):
    """make() -> in/out tensors; call(outs, ws_ptr, ws_bytes) -> rc; expected: (index into outs, reference tensor, length or None).
    -> the tensors of the call that fitted"""
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.empty(nbytes, dtype=u8, device='cuda')
    outs = make()
    rc = call(outs, ws.data_ptr(), nbytes)
    assert rc == 0, L.spg_last_error()
    torch.cuda.synchronize()
    for k, ref, m in expected:
        got = outs[k].reshape(-1) if m is None else outs[k].reshape(-1)[:m]
        assert same(got, ref), (query, k)
    short = make()
    before = [o.clone() for o in short]
    rc = call(short, ws.data_ptr(), nbytes - 1)
    assert rc != 0
    assert query.encode() in L.spg_last_error(), L.spg_last_error()
    torch.cuda.synchronize()
    for k, (o, b) in enumerate(zip(short, before)):
        assert same(o, b), (query, 'written by a refused call', k)
    return outs


def graph_inputs(n, E, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (E,), generator=g, dtype=i64).cuda()
    tgt = torch.randint(0, n, (E,), generator=g, dtype=i64).cuda()
    trans = (torch.rand(E, generator=g) < 0.4).to(u8).cuda()
    pred = torch.randint(0, max(n // 8, 1), (n,), generator=g, dtype=i32).cuda()
    return src, tgt, trans, pred, g


@pytest.mark.parametrize('n,E', SIZES)
def test_edge_units(L, n, E):
    from superpoint_graph_amd import ops
    src, tgt, trans, pred, g = graph_inputs(n, E, 1)
    graph = ops.EdgeGraph(src, tgt, n)
    exact_and_short(L, 'spg_edgegraph_workspace_bytes', L.spg_edgegraph_workspace_bytes(n, E),
                    lambda: fresh((n + 1, i32), (2 * E, i32), (2 * E, i32), (1, i32)),
                    lambda o, ws, b: L.spg_edgegraph_build(P(src), P(tgt), E, n, P(o[0]), P(o[1]), P(o[2]), P(o[3]), ws, b, stream()),
                    [(0, graph.rowptr, None), (1, graph.inc, None), (2, graph.ends, None)])

    d = 8
    emb = torch.randn(n, d, generator=g).cuda()
    weights = torch.rand(E, generator=g).cuda()
    diff, _, dl, loss = ops._edge_forward(3, emb, graph, 0, 2, 0, trans, weights, None)
    exact_and_short(L, 'spg_edge_forward_workspace_bytes', L.spg_edge_forward_workspace_bytes(E),
                    lambda: fresh((E, f32), (E, f32), (2, f64)),
                    lambda o, ws, b: L.spg_edge_forward(3, P(emb), n, d, P(graph.ends), E, 0, 2, 0, P(trans), P(weights), P(o[0]), None, P(o[1]),
                                                        P(o[2]), ws, b, stream()),
                    [(0, diff, None), (1, dl, None), (2, loss, None)])

    active = (1 - trans).contiguous()
    comp, k, size = ops.connected_components(graph, active)
    cc_call = lambda o, ws, b: L.spg_connected_components(P(graph.ends), P(active), E, n, P(o[0]), P(o[1]), P(o[2]), ws, b, stream())
    exact_and_short(L, 'spg_cc_workspace_bytes', L.spg_cc_workspace_bytes(n), lambda: fresh((n, i32), (n, i32), (1, i32)), cc_call,
                    [(0, comp, None), (1, size, k), (2, torch.tensor([k], dtype=i32, device='cuda'), None)])

    w, comp, k, size = ops.crosspartition_weights(graph, pred, trans, 5.0, return_components=True)
    exact_and_short(L, 'spg_xpart_workspace_bytes', L.spg_xpart_workspace_bytes(n, E),
                    lambda: fresh((E, f32), (n, i32), (n, i32), (1, i32)),
                    lambda o, ws, b: L.spg_xpart_weights(P(graph.ends), E, n, P(pred), P(trans), 5.0, P(o[0]), P(o[1]), P(o[2]), P(o[3]), ws, b,
                                                         stream()),
                    [(0, w, None), (1, comp, None), (2, size, k), (3, torch.tensor([k], dtype=i32, device='cuda'), None)])


@pytest.mark.parametrize('n,E', SIZES)
def test_partition_eval_units(L, n, E):
    from superpoint_graph_amd import ops
    src, tgt, trans, pred, g = graph_inputs(n, E, 2)
    graph = ops.EdgeGraph(src, tgt, n)
    n_com = max(n // 8, 1)
    index = ops.PartitionIndex(pred, n_com)
    exact_and_short(L, 'spg_partition_index_workspace_bytes', L.spg_partition_index_workspace_bytes(n, n_com),
                    lambda: fresh((n, i32), (n_com + 1, i32), (n_com, i32), (1, i32)),
                    lambda o, ws, b: L.spg_partition_index(P(pred), n, n_com, P(o[0]), P(o[1]), P(o[2]), P(o[3]), ws, b, stream()),
                    [(0, index.order, None), (1, index.offsets, None), (2, index.size, None)])

    values = torch.randint(0, 5, (n,), generator=g, dtype=i32).cuda()
    flag = torch.zeros(1, dtype=i32, device='cuda')
    freq, value = ops._component_mode(pred, values, n_com, flag)
    exact_and_short(L, 'spg_component_mode_workspace_bytes', L.spg_component_mode_workspace_bytes(n, n_com),
                    lambda: fresh((n_com, i32), (n_com, i32), (1, i32)),
                    lambda o, ws, b: L.spg_component_mode(P(pred), P(values), n, n_com, P(o[0]), P(o[1]), P(o[2]), ws, b, stream()),
                    [(0, freq, None), (1, value, None)])

    relaxed = ops._relax(graph, trans, 2, 1)
    exact_and_short(L, 'spg_relax_edges_workspace_bytes', L.spg_relax_edges_workspace_bytes(n), lambda: fresh((E, u8)),
                    lambda o, ws, b: L.spg_relax_edges(P(graph.ends), E, n, P(trans), 2, 1, P(o[0]), ws, b, stream()), [(0, relaxed, None)])


@pytest.mark.parametrize('n,E', SIZES)
def test_subgraph_units(L, n, E):
    from superpoint_graph_amd import ops
    src, tgt, _, _, g = graph_inputs(n, E, 3)
    graph = ops.EdgeGraph(src, tgt, n)
    size = (n + 1) // 2
    seeds = torch.randperm(n, generator=g).to(i64).cuda()
    sel_edg, sel_ver, n_seen, used, _ = ops.random_subgraph(graph, size, seeds)
    state_ref = torch.tensor([n_seen, used, 0], dtype=i64, device='cuda')
    exact_and_short(L, 'spg_random_subgraph_workspace_bytes', L.spg_random_subgraph_workspace_bytes(n),
                    lambda: [torch.zeros(n, dtype=u8, device='cuda'), fresh((E, u8))[0], torch.zeros(3, dtype=i64, device='cuda')],
                    lambda o, ws, b: L.spg_random_subgraph(P(graph.rowptr), P(graph.inc), P(graph.ends), E, n, size, P(seeds), n, P(o[0]), P(o[1]),
                                                           P(o[2]), ws, b, stream()),
                    [(0, sel_ver, None), (1, sel_edg, None), (2, state_ref, None)])

    rows, new_index, kept, s2, t2 = ops.induced_subgraph(graph, sel_ver, sel_edg)
    counts = torch.tensor([rows.numel(), kept.numel()], dtype=i64, device='cuda')
    exact_and_short(L, 'spg_induced_subgraph_workspace_bytes', L.spg_induced_subgraph_workspace_bytes(n, E),
                    lambda: fresh((n, i64), (n, i64), (E, i64), (E, i64), (E, i64), (2, i64)),
                    lambda o, ws, b: L.spg_induced_subgraph(P(graph.ends), E, n, P(sel_ver), P(sel_edg), P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]),
                                                            P(o[5]), ws, b, stream()),
                    [(0, rows, rows.numel()), (1, new_index, None), (2, kept, kept.numel()), (3, s2, kept.numel()), (4, t2, kept.numel()),
                     (5, counts, None)])


@pytest.mark.parametrize('n', [1, 257])
def test_prune_and_knn(L, n):
    from superpoint_graph_amd import ops
    g = torch.Generator().manual_seed(4)
    xyz = (torch.rand(n, 3, generator=g) * 4).cuda()
    rgb = torch.randint(0, 256, (n, 3), generator=g, dtype=u8).cuda()
    ref = ops.prune(xyz, 0.7, rgb=rgb)
    V = int(ref[0].shape[0])
    nbytes = L.spg_prune_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=u8, device='cuda')        # phase 2 reads what phase 1 left in the same buffer
    vox = lambda o, w, b: L.spg_prune_voxels(P(xyz), n, 0.7, P(o[0]), P(o[1]), ws.data_ptr(), b, stream())
    exact_and_short(L, 'spg_prune_workspace_bytes', nbytes, lambda: fresh((1, i64), (1, i32)), vox,
                    [(0, torch.tensor([V], dtype=i64, device='cuda'), None)])
    red = lambda o, w, b: L.spg_prune_reduce(P(xyz), P(rgb), None, None, n, V, 0, 0, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), ws.data_ptr(), b,
                                             stream())
    exact_and_short(L, 'spg_prune_workspace_bytes', nbytes, lambda: fresh((V * 3, f32), (V * 3, u8), (V, i32), (V, i32), (1, i32)), red,
                    [(0, ref[0], None), (1, ref[1], None), (2, ref[2], None), (3, ref[3], None)])

    # knn: the workspace is the larger of the build layout and the layout of one full query chunk.  With no query capacity it is
    # the build's exactly.  spg_knn_query needs all of it only where the chunk's layout is the larger one AND the chunk cannot be
    # halved (up to 64 queries); otherwise one byte less still holds a (smaller) chunk and the call must give the same result.
    k = 1 if n == 1 else 5
    for nq in (1, 257):
        q = (torch.rand(nq, 3, generator=g) * 5 - 0.5).cuda()
        idx, dist = ops.knn(xyz, k, query_xyz=q)
        build_bytes, nbytes = L.spg_knn_workspace_bytes(n, 0, 1), L.spg_knn_workspace_bytes(n, nq, 1)
        assert nbytes >= build_bytes and L.spg_knn_query_chunk(n, nq, nbytes) == nq
        ws = torch.empty(nbytes, dtype=u8, device='cuda')
        build = lambda o, w, b: L.spg_knn_build(P(xyz), n, 0.0, P(o[0]), ws.data_ptr(), b, stream())
        exact_and_short(L, 'spg_knn_workspace_bytes', build_bytes, lambda: fresh((1, i32)), build, [(0, torch.zeros(1, dtype=i32, device='cuda'), None)])
        query = lambda o, w, b: L.spg_knn_query(P(q), nq, n, k, 0, P(o[0]), P(o[1]), P(o[2]), ws.data_ptr(), b, stream())
        outs = lambda: fresh((nq * k, i32), (nq * k, f32), (1, i32))
        if nq <= 64 and nbytes > build_bytes:
            exact_and_short(L, 'spg_knn_workspace_bytes', nbytes, outs, query, [(0, idx, None), (1, dist, None)])
        else:
            for b in (nbytes, nbytes - 1):
                o = outs()
                assert query(o, None, b) == 0, L.spg_last_error()
                assert same(o[0], idx) and same(o[1], dist)
            assert nq <= 64 or 64 <= L.spg_knn_query_chunk(n, nq, nbytes - 1) < nq
    if n > k:
        idx, dist = ops.knn(xyz, k)
        ws = torch.empty(build_bytes, dtype=u8, device='cuda')
        o = fresh((1, i32), (n * k, i32), (n * k, f32))
        assert L.spg_knn_build(P(xyz), n, 0.0, P(o[0]), ws.data_ptr(), build_bytes, stream()) == 0
        assert L.spg_knn_query(None, n, n, k, 1, P(o[1]), P(o[2]), P(o[0]), ws.data_ptr(), build_bytes, stream()) == 0
        assert same(o[1], idx) and same(o[2], dist)


@pytest.mark.parametrize('n', [1, 257])
def test_sp_graph_stages(L, n):
    from superpoint_graph_amd import ops
    g = torch.Generator().manual_seed(5)
    xyz = torch.rand(n, 3, generator=g).cuda()
    n_com = n                                                  # the size query covers n_com <= n: the bound is the exact fit
    comp = torch.randperm(n, generator=g).to(i32).cuda()
    T = 0 if n < 4 else 300
    tets = torch.stack([torch.randperm(n, generator=g)[:4] for _ in range(T)]).to(i32).cuda() if T else torch.zeros(0, 4, dtype=i32, device='cuda')
    ref = ops.sp_graph(xyz, comp, n_com, tets, 0.0)
    exact_and_short(L, 'spg_spg_workspace_bytes(2, n)', L.spg_spg_workspace_bytes(2, n),
                    lambda: fresh((n_com * 3, f32), (n_com, f32), (n_com, f32), (n_com, f32), (n_com, i64)),
                    lambda o, ws, b: L.spg_spg_superpoints(P(xyz), n, P(comp), n_com, None, None, 0, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]),
                                                           None, ws, b, stream()),
                    [(0, ref['sp_centroids'], None), (1, ref['sp_length'], None), (2, ref['sp_surface'], None), (3, ref['sp_volume'], None),
                     (4, ref['sp_point_count'], None)])
    # raw interface pairs: from the tetrahedra, or one hand-made pair for the smallest size (n = 1 has no tetrahedron)
    if T:
        keys = torch.empty(12 * T, dtype=i64, device='cuda')
        cnt = torch.zeros(1, dtype=i64, device='cuda')
        assert L.spg_spg_tet_edges(P(tets), T, P(comp), P(keys), 12 * T, P(cnt), stream()) == 0
        n_raw, n_edg, n_sedg = int(cnt.item()), int(ref['edges'].numel()), int(ref['seg_off'].numel()) - 1
        assert n_raw > 256 and n_edg > 256
    else:
        keys, n_raw, n_edg, n_sedg = torch.zeros(1, dtype=i64, device='cuda'), 1, 1, 1
    one = lambda v: torch.tensor([v], dtype=i64, device='cuda')
    # (the wrapper does not return the unique keys: their number here, and what the next stage makes of them, below)
    o = exact_and_short(L, 'spg_spg_workspace_bytes(0, n)', L.spg_spg_workspace_bytes(0, n_raw), lambda: fresh((n_raw, i64), (n_raw, i64), (1, i64)),
                        lambda o, ws, b: L.spg_spg_unique_edges(P(keys), n_raw, P(xyz), P(comp), n_com, 0.0, P(o[0]), P(o[1]), P(o[2]), ws, b,
                                                                stream()),
                        [(2, one(n_edg), None)])
    edge_keys, cc_keys = o[0], o[1]
    exact_and_short(L, 'spg_spg_workspace_bytes(1, n)', L.spg_spg_workspace_bytes(1, n_edg),
                    lambda: fresh((n_edg, i64), (n_edg, i64), (n_edg, i64), (n_edg + 1, i64), (1, i64)),
                    lambda o, ws, b: L.spg_spg_group_edges(P(cc_keys), P(edge_keys), n_edg, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), ws, b,
                                                           stream()),
                    [(4, one(n_sedg), None)] + ([(1, ref['edges'], n_edg), (3, ref['seg_off'], n_sedg + 1)] if T else []))


@pytest.mark.parametrize('n,T', [(3, 1), (1300, 1), (1300, 100)])
def test_plane_units(L, n, T):
    from superpoint_graph_amd import ops
    g = torch.Generator().manual_seed(6)
    xyz = (torch.rand(n, 3, generator=g) * torch.tensor([10.0, 8.0, 0.3])).cuda()      # z < 0.3: every point is a low point
    subsets = torch.from_numpy(ops.ransac_subsets(n, T, 0)).to(i32).cuda()
    ref = ops.plane_elevation(xyz, subsets=subsets)
    n_low = ref['n_low']
    assert n_low == n
    word = lambda *v: torch.tensor(v, dtype=i32, device='cuda')
    exact_and_short(L, 'spg_plane_workspace_bytes(n, -1, 0)', L.spg_plane_workspace_bytes(n, -1, 0), lambda: fresh((n, i32), (1, i32), (1, i32)),
                    lambda o, ws, b: L.spg_plane_low(P(xyz), n, 0.5, P(o[0]), P(o[1]), P(o[2]), ws, b, stream()),
                    [(0, ref['low_index'], n_low), (1, word(n_low), None), (2, word(0), None)])
    low = ref['low_index'].contiguous()
    # (the fit ORs into its error word and does not clear it: the caller hands it over as zero)
    exact_and_short(L, 'spg_plane_workspace_bytes(n, n_low, trials)', L.spg_plane_workspace_bytes(n, n_low, T),
                    lambda: fresh((n, f32), (2, f64), (1, f64), (1, f32), (n_low, u8), (2, i32)) + [torch.zeros(1, dtype=i32, device='cuda')],
                    lambda o, ws, b: L.spg_plane_fit(P(xyz), n, P(low), n_low, P(subsets), T, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(o[5]),
                                                     P(o[6]), ws, b, stream()),
                    [(0, ref['elevation'], None), (1, ref['coef'], None), (2, ref['intercept'], None), (3, ref['threshold'], None),
                     (4, ref['inlier_mask'], None), (5, word(ref['n_trials'], ref['best_trial']), None), (6, word(0), None)])
