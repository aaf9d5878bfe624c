"""--ptn_norm layer|group of the learned partition (reference learning/pointnet.py:24-49, 75-118; supervized_partition.py:98-99,
411-421): the product classes build the reference's module sequence under the reference's state_dict keys, so that its
checkpoints load strictly.  CPU only: nothing is launched."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN
from groupnorm_golden import build_model, cli_args, state_of

NORM_SLOTS = {'stn.convs': (1, 4), 'stn.fcs': (1, 4), 'ptn.convs': (1, 4), 'ptn.fcs': (1, 4, 7)}
WIDTHS = {'stn.convs': (16, 64), 'stn.fcs': (32, 16), 'ptn.convs': (32, 128), 'ptn.fcs': (34, 32, 32)}


def _create(norm, n_group=2):
    from superpoint_graph_amd.supervized_partition.supervized_partition import create_model
    return create_model(cli_args(norm, n_group))


@pytest.mark.parametrize('norm', ['layer', 'group'])
def test_create_model_loads_the_reference_state_strictly(norm):
    model, state = _create(norm), state_of(norm)
    own = model.state_dict()
    assert list(own.keys()) == list(state.keys())
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in state.items()}
    model.load_state_dict(state, strict=True)
    assert all(torch.equal(model.state_dict()[k], v) for k, v in state.items())
    assert own['ptn.convs.1.weight'].shape == (32,) and not any('running' in k or 'num_batches' in k for k in own)


@pytest.mark.parametrize('norm, stn_groups, ptn_groups', [('layer', 1, 1), ('group', 2, 1)])
def test_module_sequence_is_the_references(norm, stn_groups, ptn_groups):
    """create_model hands ptn_n_group to the STN only, as the reference does (supervized_partition.py:415 vs :421)."""
    model = _create(norm)
    for path, slots in NORM_SLOTS.items():
        seq = model.get_submodule(path)
        for slot, width in zip(slots, WIDTHS[path]):
            m = seq[slot]
            assert isinstance(m, nn.GroupNorm) and m.num_channels == width and m.affine and m.eps == 1e-5, (path, slot, m)
            assert m.num_groups == (stn_groups if path.startswith('stn') else ptn_groups), (path, slot, m)
            assert isinstance(seq[slot - 1], (nn.Conv1d, nn.Linear)) and isinstance(seq[slot + 1], nn.ReLU)
    assert isinstance(model.ptn.fcs[9], nn.Linear) and len(model.ptn.fcs) == 10 and isinstance(model.stn.proj, nn.Linear)


def test_classes_take_n_group():
    model = build_model('group')
    assert all(m.num_groups == 2 for m in model.modules() if isinstance(m, nn.GroupNorm))
    assert sum(isinstance(m, nn.GroupNorm) for m in model.modules()) == 9
    with pytest.raises(ValueError):
        from superpoint_graph_amd.learning import pointnet
        pointnet.STNkD(2, [16, 64], [32, 16], norm='instance')


def test_batch_models_keep_their_keys():
    """norm='batch' has the keys of today: those of the BatchNorm embedder's own golden (tests/golden/local_embedder.npz)."""
    g = np.load(os.path.join(GOLDEN, 'local_embedder.npz'))
    today = [k[7:] for k in g.files if k.startswith('state0/')]
    model = _create('batch')
    assert sorted(model.state_dict().keys()) == sorted(today)
    assert sum(isinstance(m, nn.BatchNorm1d) for m in model.modules()) == 9
    assert not any(isinstance(m, nn.GroupNorm) for m in model.modules())


def test_geof_vertex_values_are_refused():
    from superpoint_graph_amd.supervized_partition.supervized_partition import create_model
    for v in ('geof', 'geofrgb'):
        args = cli_args('layer')
        args.ver_value = v
        with pytest.raises(NotImplementedError, match='geof'):
            create_model(args)
