"""CPU: host-side logic of the product package and the C-ABI library (loads, exports every declared
symbol, answers size queries) -- no kernels are launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, build_model, load_golden
from oracle import spg_oracle as O
from superpoint_graph_amd import _lib, ops, synth
from superpoint_graph_amd.learning import ecc, spg


def test_library_exports_every_declared_symbol(hip):
    hdr = open(os.path.join(ROOT, 'include', 'spg_hip.h')).read()
    declared = set(re.findall(r'\b(spg_[a-z0-9_]+)\s*\(', hdr))
    declared -= {'spg_pointnet_cfg', 'spg_eccrnn_cfg'}
    assert declared, 'no declarations parsed'
    for name in sorted(declared):
        assert hasattr(hip, name), f'{name} declared in include/spg_hip.h but not exported'
        assert name in _lib.SIGNATURES, f'{name} has no ctypes signature'
    assert hip.spg_version() == 200


def test_size_queries(hip):
    cfg = ops.make_pointnet_cfg(14, 14, 1, 128, [64, 64, 128], [128, 64], [64, 64, 128, 128, 256], [256, 64, 32])
    assert hip.spg_pointnet_num_layers(ctypes.byref(cfg)) == 14
    train, ev = hip.spg_pointnet_workspace_bytes(ctypes.byref(cfg), 1000, 1), hip.spg_pointnet_workspace_bytes(ctypes.byref(cfg), 1000, 0)
    assert train > ev > 0
    assert hip.spg_pointnet_bwd_workspace_bytes(ctypes.byref(cfg), 1000) > 0
    bad = ops.make_pointnet_cfg(14, 14, 1, 4096, [64], [64], [64], [32])
    assert hip.spg_pointnet_workspace_bytes(ctypes.byref(bad), 10, 1) == 0 and b'npts' in hip.spg_last_error()
    c2 = ops.make_eccrnn_cfg(32, 10, True, True, True, True, [13, 32, 128, 64, 1024], 2, False)
    assert hip.spg_eccrnn_workspace_bytes(ctypes.byref(c2), 1000, 5000, 1) > 0
    assert hip.spg_graph_workspace_bytes(1000, 1000, 5000) >= 4 * (2 * 1001 + 3 * 5000)
    # retired spg_tune keys (their code paths are gone): switching one on fails loudly, 0 stays accepted
    for k in (9, 12, 13, 16, 19):
        assert hip.spg_tune(k, 1) == -1, k
        assert hip.spg_tune(k, 0) >= 0, k


def test_graphconvinfo_bit_exact_and_collate():
    scenes = [synth.scene(s, n_sp=60, n_edges=240, small_frac=0.1) for s in (3, 4, 5)]
    targets, GIs, (meta, flag, clouds, diam) = spg.eccpc_collate([spg.sample_from_scene(s, f'sc{i}') for i, s in enumerate(scenes)])
    col = synth.collate_numpy(scenes)
    idxn, degs, ef, ei = O.set_batch(col['edge_lists'], col['vcounts'], col['edge_feats'])
    gi = GIs[0]
    b_idxn, b_idxe, b_degs, b_degs_gpu, b_ef = gi.get_buffers()
    assert b_idxn.dtype == torch.int64 and b_degs.dtype == torch.int64 and b_idxe is None and b_degs_gpu is None
    assert np.array_equal(b_idxn.numpy(), idxn) and np.array_equal(b_degs.numpy(), degs)
    assert np.array_equal(b_ef.numpy(), ef) and np.array_equal(gi.get_pyg_buffers().numpy(), ei)
    assert targets.shape == (180, 15) and flag.shape == (180,) and len(meta) == 180
    assert clouds.shape[0] == int((flag == 0).sum()) == diam.shape[0]
    assert np.array_equal(flag.numpy(), col['clouds_flag']) and np.array_equal(targets.numpy(), col['targets'])


def test_golden_index_buffers_from_graphs():
    spec, batch, state0, g = load_golden('s3dis_gru10_matrix')
    graphs = [spg.SuperpointGraph(int(g[f'graph/{i}/n']), g[f'graph/{i}/edges'], True, {'f': list(g[f'graph/{i}/feats'])}) for i in range(2)]
    gi = ecc.GraphConvInfo(graphs, spg.cloud_edge_feats)
    assert torch.equal(gi._idxn, batch['idxn']) and torch.equal(gi._degrees, batch['degs'])
    assert torch.equal(gi._edge_indexes, batch['edge_indexes']) and torch.equal(gi._edgefeats, batch['edgefeats'])


def test_state_dict_keys_and_init_match_reference():
    for tag in ('s3dis_gru10_matrix', 'vector_gru4_small', 'lstm3_matrix_small'):
        spec, batch, state0, g = load_golden(tag)
        torch.manual_seed(1)
        model = build_model(spec)
        sd = model.state_dict()
        assert sorted(sd.keys()) == sorted(state0.keys())
        for k, v in state0.items():
            assert tuple(sd[k].shape) == tuple(v.shape), k
        model.load_state_dict(state0)           # reference checkpoints load (learning/main.py:403)
        # the golden state perturbed BN / STN-proj only: every other tensor must equal a fresh seed-1 init
        torch.manual_seed(1)
        fresh = build_model(spec).state_dict()
        same = [k for k in state0 if 'weight_' in k or '.ig.' in k or '_fnet.0.' in k or 'convs.0.weight' in k]
        assert same
        for k in same:
            assert torch.equal(fresh[k], state0[k]), k


def test_product_path_fails_loudly_without_gpu():
    spec, batch, state0, g = load_golden('vector_gru4_small')
    model = build_model(spec, state0)
    with pytest.raises(RuntimeError, match='no CPU path'):
        model.ptn(batch['clouds'], batch['clouds_global'])
    gi = ecc.GraphConvInfo.from_buffers(batch['idxn'], batch['degs'], batch['edgefeats'])
    model.ecc.set_info([gi], cuda=False)
    with pytest.raises(RuntimeError, match='no CPU path'):
        model.ecc(torch.zeros(batch['degs'].numel(), 32))
    with pytest.raises(RuntimeError):
        ecc.GraphConvFunction.apply(torch.zeros(4, 3), torch.zeros(2, 3), 3, 3, torch.zeros(2, dtype=torch.long), None,
                                    torch.tensor([1, 1, 0, 0]), None, 1e20)


def test_model_config_dsl():
    from superpoint_graph_amd.learning import graphnet
    net = graphnet.GraphNetwork('gru_10_0,f_13', 32, [13, 32, 128, 64], 1, 0, 2, 30000, use_pyg=0, cuda=0)
    assert sum(p.numel() for p in net.parameters()) == 90573
    net = graphnet.GraphNetwork('gru_10,f_8', 32, [13, 32, 128, 64], 1, 0, 2, 30000, use_pyg=0, cuda=0)
    assert net.gconvs[0]._fnet[-1].weight.shape == (32, 64)
    net = graphnet.GraphNetwork('lstm_3_0,f_8', 32, [13, 32, 128, 64], 1, 0, 2, 30000, use_pyg=0, cuda=0)
    assert net.gconvs[0]._isLSTM and net.gconvs[0]._cell.weight_ih.shape == (128, 32) and net._modules['1'].in_features == 128
    with pytest.raises(NotImplementedError):
        graphnet.GraphNetwork('crf_3', 32, [13, 32], use_pyg=0)
    with pytest.raises(NotImplementedError):
        graphnet.GraphNetwork('xyz_3', 32, [13, 32], use_pyg=0)


def test_philox_oracle_known_answers():
    """The counter-based generator behind `--loader_rng device`: the three known-answer vectors of the Random123
    distribution (kat_vectors: philox4x32 10 rounds)."""
    from oracle.philox_oracle import philox4x32_10
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(x) for x in philox4x32_10(*ctr, *key))
        assert got == want


def test_superpoint_graph_igraph_semantics():
    """The igraph.Graph semantics `SuperpointGraph` stands in for (class docstring), against hand-written expected values
    taken from python-igraph's documented behaviour -- the stand-in is also what the CLI golden was generated with
    (oracle/gen_main_golden.py installs it as igraph.Graph for the reference run), so a deviation from real igraph would
    otherwise be invisible to every other test."""
    from superpoint_graph_amd.learning.spg import SuperpointGraph, random_neighborhoods, k_big_enough
    # directed graph on 6 vertices; edge attribute 'f' = edge id, vertex attribute 'v' = letters, 's' = sizes
    edges = [(0, 1), (1, 2), (2, 4), (4, 1), (3, 0), (5, 4)]
    G = SuperpointGraph(6, edges, True, {'f': [10, 11, 12, 13, 14, 15]}, {'v': list('abcdef'), 's': [50, 5, 60, 70, 8, 90]})
    assert G.vcount() == 6 and G.get_edgelist() == edges and G.indegree(G.vs) == [1, 2, 1, 0, 2, 0]
    assert G.es.attributes() == ['f'] and G.es[[3, 0]].get_attribute_values('f') == [13, 10]
    assert G.vs[2]['v'] == 'c' and G.vs['s'] == [50, 5, 60, 70, 8, 90]
    # Graph.neighborhood(vertices, order) with the default mode='all': direction ignored, the vertex itself included.
    #   igraph docs example shape: g.neighborhood([v], order=1) -> [[v, neighbours...]]
    nb1 = G.neighborhood([0], 1)
    assert nb1[0][0] == 0 and sorted(nb1[0]) == [0, 1, 3]                 # 0->1 (out) and 3->0 (in) both count
    assert sorted(G.neighborhood([2], 1)[0]) == [1, 2, 4]
    assert sorted(G.neighborhood([0], 2)[0]) == [0, 1, 2, 3, 4]           # via 1: 2 and 4 (4->1 counts); 5 is three steps away
    assert [sorted(x) for x in G.neighborhood([5, 3], 1)] == [[4, 5], [0, 3]]
    assert sorted(G.neighborhood([5], 0)[0]) == [5]
    # Graph.permute_vertices(perm): "vertex k of the original graph becomes vertex perm[k] in the new graph"
    P = G.permute_vertices([2, 0, 1, 5, 4, 3])
    assert P.get_edgelist() == [(2, 0), (0, 1), (1, 4), (4, 0), (5, 2), (3, 4)]      # same edges, same order, relabelled
    assert P.vs['v'] == ['b', 'c', 'a', 'f', 'e', 'd'] and P.es.get_attribute_values('f') == [10, 11, 12, 13, 14, 15]
    # Graph.subgraph(vertices) (induced_subgraph): survivors renumbered in increasing order of their old ids
    S = G.subgraph([1, 2, 4])
    assert S.vcount() == 3 and S.vs['v'] == ['b', 'c', 'e']
    assert sorted(zip(S.get_edgelist(), S.es.get_attribute_values('f'))) == [((0, 1), 11), ((1, 2), 12), ((2, 0), 13)]
    S2 = G.subgraph([4, 1, 2])                                            # the order the ids are passed in does not matter in igraph
    assert S2.vs['v'] == ['b', 'c', 'e'] and sorted(S2.get_edgelist()) == sorted(S.get_edgelist())
    assert G.subgraph([0, 5]).get_edgelist() == []                        # no edge between the survivors
    # the two callers (reference learning/spg.py:114-127)
    import random
    random.seed(0)
    R = random_neighborhoods(G, 1, 1)
    assert R.vcount() in (2, 3, 4) and set(R.vs['v']) <= set('abcdef')
    K = k_big_enough(G, 40, 2)             # sizes 50, 5, 60, 70, ...: the prefix holding 2 superpoints of >= 40 points = ids 0..2
    assert K.vs['v'] == ['a', 'b', 'c'] and K.get_edgelist() == [(0, 1), (1, 2)]


def test_concat_edge_attribute_skips_edgeless_graphs():
    """GraphConvInfo.set_batch_device's concatenation of per-graph edge attributes: graphs without edges contribute arrays of
    unknown trailing shape -- (0, 0) from SuperpointGraph, (0,) from an igraph value list -- and are skipped."""
    from superpoint_graph_amd.learning.ecc.GraphConvInfo import _concat_edge_attribute
    a, b = np.arange(6, dtype=np.float32).reshape(2, 3), np.arange(9, dtype=np.float32).reshape(3, 3)
    out = _concat_edge_attribute([a, np.zeros((0, 0), dtype=np.float32), b, np.asarray([])])
    assert out.shape == (5, 3) and np.array_equal(out[:2], a) and np.array_equal(out[2:], b)
    assert _concat_edge_attribute([np.zeros((0, 0)), a]) is a
    assert _concat_edge_attribute([np.asarray([]), np.zeros((0, 0))]).shape == (0, 0)


def test_bench_refuses_to_report_fewer_ranks_than_asked_for():
    """`python bench.py --gpus N` with no torchrun environment starts its own ranks -- and on a node with fewer
    than N GPUs (here: none) it must fail loudly instead of printing the line of a smaller job."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '8', '--steps', '2', '--warmup', '1'], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and 'refusing' in out.stderr
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith('{')]


def test_graphconvinfo_rejects_a_part_hint_that_is_not_closed_under_edges():
    """GraphConvInfo.from_buffers(parts=...) is a promise to the one-launch recurrence (rounds of whole scenes); a hint
    with an edge across a boundary is rejected on the host before the device graph is built."""
    import torch
    from superpoint_graph_amd.learning import ecc
    # 4 nodes, edges (src -> tgt) sorted by target: 1->0, 0->1, 3->2, 2->3: two components {0,1}, {2,3}
    idxn, degs = torch.tensor([1, 0, 3, 2]), torch.tensor([1, 1, 1, 1])
    ef = torch.zeros(4, 13)
    ecc.GraphConvInfo.from_buffers(idxn, degs, ef, parts=[0, 2, 4])._validate()
    with pytest.raises(ValueError, match='crosses a part boundary'):
        ecc.GraphConvInfo.from_buffers(idxn, degs, ef, parts=[0, 1, 4])._validate()
    with pytest.raises(ValueError, match='non-decreasing node offsets'):
        ecc.GraphConvInfo.from_buffers(idxn, degs, ef, parts=[0, 2, 3])._validate()
