"""GPU: the supervised loader's neighbourhood sub-sampling on the device (csrc/spg_sample.hip, ops.ResidentSPG / sample_spg,
spg.DeviceGraphCache / DeviceSampledGraph, `--spg_sample_device`) against the host path -- SuperpointGraph.permute_vertices,
random_neighborhoods, k_big_enough under the same random seed (tests/spg_sample_cases.py: host_sample), never against the new
code: integers exactly, feature rows bit for bit; then through `loader`, the device collate and one short CLI run."""
import random

import numpy as np
import pytest
import torch

import main_fixture
import spg_sample_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _resident(case):
    from superpoint_graph_amd import ops
    return ops.ResidentSPG(case['edges'], case['feats'] if len(case['edges']) else None, case['sizes'], case['n'])


def _sample(case, perm, centres, g=None):
    from superpoint_graph_amd import ops
    return ops.sample_spg(g or _resident(case), perm, centres, case['order'], case['minpts'], case['hardcutoff'])


@pytest.mark.parametrize('name', C.NAMES)
def test_sample_equals_the_host_path(hip, name):
    case, perm, centres, host = C.cases()[name]
    s = _sample(case, perm, centres)
    assert (s.n, s.E) == (len(host['vids']), len(host['kept']))
    assert np.array_equal(s.vids.numpy(), host['vids'])
    assert np.array_equal(s.degs.numpy(), host['degs'])
    assert np.array_equal(s.edges.cpu().numpy(), host['edges'])
    assert np.array_equal(s.kept.cpu().numpy(), host['kept'])
    if len(case['edges']):
        assert np.array_equal(s.feats.cpu().numpy().view(np.uint32), host['feats'].view(np.uint32))


def test_bad_centre_and_bad_perm_raise(hip):
    case, perm, centres, _ = C.cases()['blocks_257']
    g = _resident(case)
    with pytest.raises(IndexError):
        _sample(case, perm, centres[:-1] + [case['n']], g)
    with pytest.raises(IndexError):
        _sample(case, None, [-1], g)
    twice = list(perm)
    twice[5] = twice[200]
    with pytest.raises(ValueError):
        _sample(case, twice, centres, g)
    with pytest.raises(ValueError):
        _sample(case, perm[:-1] + [case['n']], centres, g)
    s = _sample(case, perm, centres, g)                                   # the graph serves further samples
    assert np.array_equal(s.vids.numpy(), C.cases()['blocks_257'][3]['vids'])


@pytest.mark.parametrize('name', ['s3dis', 'hub300'])
def test_two_runs_return_identical_bytes(hip, name):
    case, perm, centres, _ = C.cases()[name]
    g = _resident(case)
    a, b = _sample(case, perm, centres, g), _sample(case, perm, centres, g)
    for key in ('vids', 'degs', 'edges', 'kept', 'feats'):
        assert torch.equal(getattr(a, key), getattr(b, key)), key


def test_device_tensors_as_perm_and_centres(hip):
    case, perm, centres, host = C.cases()['blocks_1025']
    s = _sample(case, torch.tensor(perm, device=DEV), torch.tensor(centres, device=DEV))
    assert np.array_equal(s.vids.numpy(), host['vids']) and np.array_equal(s.kept.cpu().numpy(), host['kept'])


@pytest.mark.parametrize('name', ['n2_one_edge', 'blocks_257'])
def test_workspace_of_exactly_the_queried_size(hip, name):
    """The convention of the partition units: a buffer of exactly spg_sample_spg_workspace_bytes is enough
    and gives what the wrapper gives; with one byte less the call is refused before anything is written."""
    case, perm, centres, _ = C.cases()[name]
    g = _resident(case)
    ref = _sample(case, perm, centres, g)
    n, E, i64 = g.n, g.E, torch.int64
    perm_d, centres_d = torch.tensor(perm, device=DEV), torch.tensor(centres, device=DEV)
    nbytes = hip.spg_sample_spg_workspace_bytes(n, E)
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def call(ws_bytes):
        outs = [torch.full((k,), -7, dtype=i64, device=DEV) for k in (n, 2 * E, E, n, 3)] + [torch.full((E, C.F), -7.0, device=DEV)]
        vids, edges, kept, degs, head, feats = outs
        rc = hip.spg_sample_spg(g.graph.ends.data_ptr(), E, n, perm_d.data_ptr(), centres_d.data_ptr(), len(centres), g.sizes.data_ptr(),
                                g.feats.data_ptr(), C.F, case['order'], case['minpts'], case['hardcutoff'], vids.data_ptr(), edges.data_ptr(),
                                kept.data_ptr(), feats.data_ptr(), degs.data_ptr(), head.data_ptr(), ws.data_ptr(), ws_bytes,
                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, outs
    rc, (vids, edges, kept, degs, head, feats) = call(nbytes)
    assert rc == 0, hip.spg_last_error()
    assert head.tolist() == [ref.n, ref.E, 0]
    assert torch.equal(vids[:ref.n].cpu(), ref.vids) and torch.equal(degs[:ref.n].cpu(), ref.degs)
    assert torch.equal(edges[:2 * ref.E].view(-1, 2), ref.edges) and torch.equal(kept[:ref.E], ref.kept) and torch.equal(feats[:ref.E], ref.feats)
    rc, outs = call(nbytes - 1)
    assert rc != 0 and b'spg_sample_spg_workspace_bytes' in hip.spg_last_error()
    assert all(bool((o == -7).all()) for o in outs)


# ---------------------------------------------------------------------------------------------------------------------
# through the loader, the collate and the CLI
# ---------------------------------------------------------------------------------------------------------------------
SUBSAMPLE = ['--spg_augm_nneigh', '2', '--spg_augm_order', '1', '--spg_augm_hardcutoff', '8']


def _loader_setup():
    from superpoint_graph_amd.learning import main as cli
    from superpoint_graph_amd.learning import spg
    args = cli.parse_args(['--dataset', 'x'] + main_fixture.CLI + SUBSAMPLE)
    args.cuda = 1
    train, _ = main_fixture.make_dataset(0)
    entries = [spg.spg_to_graph(*spg.spg_from_arrays(args, g, name)) for name, g, _ in train[:2]]
    store = spg.MemoryPointStore({name: pts for name, _, pts in train[:2]})
    return args, entries, spg.DevicePointCache(store, torch.device(DEV, torch.cuda.current_device())), spg.DeviceGraphCache()


def _samples(args, entries, cache, graphs, train):
    from superpoint_graph_amd.learning import spg
    random.seed(7); np.random.seed(8)
    return [spg.loader(e, train, args, None, test_seed_offset=3, device_cache=cache, device_graphs=graphs) for e in entries]


@pytest.mark.parametrize('train', [True, False])
def test_loader_with_and_without_device_graphs(hip, train):
    args, entries, cache, graphs = _loader_setup()
    host = _samples(args, entries, cache, None, train)
    dev = _samples(args, entries, cache, graphs, train)
    for (t_h, G_h, meta_h, flag_h, clouds_h, diam_h), (t_d, G_d, meta_d, flag_d, clouds_d, diam_d), (G, _) in zip(host, dev, entries):
        assert (G_h.vcount() < G.vcount()) == train                       # the settings really sub-sample these scenes
        assert np.array_equal(np.asarray(t_d), np.asarray(t_h)) and meta_d == meta_h
        assert np.array_equal(np.asarray(flag_d), np.asarray(flag_h))
        assert torch.equal(clouds_d, clouds_h) and torch.equal(diam_d, diam_h)
        assert G_d.vcount() == G_h.vcount() and G_d.indegree() == G_h.indegree()
        assert np.array_equal(G_d.edges.cpu().numpy(), np.asarray(G_h._edges))
        assert G_d.get_edgelist() == G_h.get_edgelist()
        assert np.array_equal(G_d.feats.cpu().numpy().view(np.uint32), np.asarray(G_h.edge_attribute_array('f'), dtype=np.float32).view(np.uint32))


def test_collate_over_device_samples(hip):
    from superpoint_graph_amd.learning import spg
    args, entries, cache, graphs = _loader_setup()
    _, gis_h, _ = spg.eccpc_collate(_samples(args, entries, cache, None, True), device_batch=True)
    _, gis_d, _ = spg.eccpc_collate(_samples(args, entries, cache, graphs, True), device_batch=True)
    h, d = gis_h[0], gis_d[0]
    assert d._parts == h._parts and d._idxe is None
    assert torch.equal(d._idxn, h._idxn) and d._idxn.is_cuda
    assert torch.equal(d._degrees, h._degrees) and not d._degrees.is_cuda
    assert torch.equal(d._degrees_gpu, h._degrees_gpu)
    assert torch.equal(d._edgefeats.view(torch.int32), h._edgefeats.view(torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(d.extras_dev, h.extras_dev) if a is not None) and len(d.extras_dev) == len(h.extras_dev)


def test_cli_losses_are_equal_bit_for_bit(hip, tmp_path):
    from superpoint_graph_amd.learning import datasets
    from superpoint_graph_amd.learning import main as cli
    train, test = main_fixture.make_dataset(0)
    datasets.register_memory_dataset('memtest_sample', [(n, g) for n, g, _ in train], [(n, g) for n, g, _ in test], [],
                                     {name: pts for name, _, pts in train + test}, main_fixture.N_CLASSES, 14)
    losses = {}
    for flag in ('0', '1'):
        session = cli.main(['--dataset', 'memtest_sample', '--odir', str(tmp_path / flag)] + main_fixture.CLI + SUBSAMPLE +
                           ['--epochs', '1', '--test_multisamp_n', '1', '--spg_sample_device', flag])
        torch.cuda.synchronize()
        losses[flag] = ([float(x[0]) for x in session.iter_log], [float(x) for x in session.eval_log])
    print('training / evaluation losses, host sub-sampling:  ', losses['0'])
    print('training / evaluation losses, device sub-sampling:', losses['1'])
    assert len(losses['0'][0]) == 2 and np.all(np.isfinite(losses['0'][0]))
    assert losses['1'] == losses['0']
