"""The parameter plumbing between the modules and the C ABI (superpoint_graph_amd/learning/_layers.py), on the CPU and without
the library: which tensors every layer hands over and in what order, the autograd input order, where the gradients land in
FlatParameters mode, the cells' state_dict keys and what the walker over a Sequential refuses.

The literal tables below were recorded from commit 9e711b0 (the parent of the model-glue refactor: `_groups_tensors()` /
`_flat_params()` of PointNet and STNkD, `_cfg_and_groups()` / `_flat_params()` of RNNGraphConvModule, `state_dict()` of the
cells), tensors mapped to their names by identity."""
import pytest
import torch
import torch.nn as nn

from superpoint_graph_amd.flat import FlatParameters
from superpoint_graph_amd.learning import _layers, graphnet, modules, pointnet

PRODUCTION = ([64, 64, 128, 128, 256], [256, 64, 32], [64, 64, 128], [128, 64], 14)


# one row per line: weight, bias, norm.weight, norm.bias, running_mean, running_var ('-': None); a cell: its six parameters
STN_ROWS = '''
convs.0.weight convs.0.bias convs.1.weight convs.1.bias convs.1.running_mean convs.1.running_var
convs.3.weight convs.3.bias convs.4.weight convs.4.bias convs.4.running_mean convs.4.running_var
convs.6.weight convs.6.bias convs.7.weight convs.7.bias convs.7.running_mean convs.7.running_var
fcs.0.weight fcs.0.bias fcs.1.weight fcs.1.bias fcs.1.running_mean fcs.1.running_var
fcs.3.weight fcs.3.bias fcs.4.weight fcs.4.bias fcs.4.running_mean fcs.4.running_var
proj.weight proj.bias - - - -'''
NOSTN_ROWS = '''
convs.0.weight convs.0.bias convs.1.weight convs.1.bias convs.1.running_mean convs.1.running_var
convs.3.weight convs.3.bias convs.4.weight convs.4.bias convs.4.running_mean convs.4.running_var
convs.6.weight convs.6.bias convs.7.weight convs.7.bias convs.7.running_mean convs.7.running_var
convs.9.weight convs.9.bias convs.10.weight convs.10.bias convs.10.running_mean convs.10.running_var
convs.12.weight convs.12.bias convs.13.weight convs.13.bias convs.13.running_mean convs.13.running_var
fcs.0.weight fcs.0.bias fcs.1.weight fcs.1.bias fcs.1.running_mean fcs.1.running_var
fcs.3.weight fcs.3.bias fcs.4.weight fcs.4.bias fcs.4.running_mean fcs.4.running_var
fcs.7.weight fcs.7.bias - - - -'''
POINTNET_ROWS = '''
stn.convs.0.weight stn.convs.0.bias stn.convs.1.weight stn.convs.1.bias stn.convs.1.running_mean stn.convs.1.running_var
stn.convs.3.weight stn.convs.3.bias stn.convs.4.weight stn.convs.4.bias stn.convs.4.running_mean stn.convs.4.running_var
stn.convs.6.weight stn.convs.6.bias stn.convs.7.weight stn.convs.7.bias stn.convs.7.running_mean stn.convs.7.running_var
stn.fcs.0.weight stn.fcs.0.bias stn.fcs.1.weight stn.fcs.1.bias stn.fcs.1.running_mean stn.fcs.1.running_var
stn.fcs.3.weight stn.fcs.3.bias stn.fcs.4.weight stn.fcs.4.bias stn.fcs.4.running_mean stn.fcs.4.running_var
stn.proj.weight stn.proj.bias - - - -''' + NOSTN_ROWS
CELL_ROW = '''
_cell.weight_ih _cell.weight_hh _cell.bias_ih _cell.bias_hh _cell.ig.weight _cell.ig.bias'''
GRU_ROWS = '''
_fnet.0.weight _fnet.0.bias - - - -
_fnet.2.weight _fnet.2.bias - - - -
_fnet.4.weight _fnet.4.bias _fnet.5.weight _fnet.5.bias _fnet.5.running_mean _fnet.5.running_var
_fnet.7.weight _fnet.7.bias - - - -''' + CELL_ROW
LSTM_ROWS = '''
_fnet.0.weight _fnet.0.bias - - - -
_fnet.2.weight _fnet.2.bias - - - -
_fnet.4.weight _fnet.4.bias - - - -
_fnet.6.weight _fnet.6.bias - - - -''' + CELL_ROW

STN_FLAT = ('convs.0.weight convs.0.bias convs.1.weight convs.1.bias convs.3.weight convs.3.bias convs.4.weight convs.4.bias '
            'convs.6.weight convs.6.bias convs.7.weight convs.7.bias fcs.0.weight fcs.0.bias fcs.1.weight fcs.1.bias '
            'fcs.3.weight fcs.3.bias fcs.4.weight fcs.4.bias proj.weight proj.bias')
NOSTN_FLAT = ('convs.0.weight convs.0.bias convs.1.weight convs.1.bias convs.3.weight convs.3.bias convs.4.weight convs.4.bias '
              'convs.6.weight convs.6.bias convs.7.weight convs.7.bias convs.9.weight convs.9.bias convs.10.weight convs.10.bias '
              'convs.12.weight convs.12.bias convs.13.weight convs.13.bias fcs.0.weight fcs.0.bias fcs.1.weight fcs.1.bias '
              'fcs.3.weight fcs.3.bias fcs.4.weight fcs.4.bias fcs.7.weight fcs.7.bias')
POINTNET_FLAT = ('stn.convs.0.weight stn.convs.0.bias stn.convs.1.weight stn.convs.1.bias stn.convs.3.weight stn.convs.3.bias '
                 'stn.convs.4.weight stn.convs.4.bias stn.convs.6.weight stn.convs.6.bias stn.convs.7.weight stn.convs.7.bias '
                 'stn.fcs.0.weight stn.fcs.0.bias stn.fcs.1.weight stn.fcs.1.bias stn.fcs.3.weight stn.fcs.3.bias '
                 'stn.fcs.4.weight stn.fcs.4.bias stn.proj.weight stn.proj.bias ' + NOSTN_FLAT)
CELL_FLAT = ' _cell.weight_ih _cell.weight_hh _cell.bias_ih _cell.bias_hh _cell.ig.weight _cell.ig.bias'
GRU_FLAT = ('_fnet.0.weight _fnet.0.bias _fnet.2.weight _fnet.2.bias _fnet.4.weight _fnet.4.bias _fnet.5.weight _fnet.5.bias '
            '_fnet.7.weight _fnet.7.bias' + CELL_FLAT)
LSTM_FLAT = '_fnet.0.weight _fnet.0.bias _fnet.2.weight _fnet.2.bias _fnet.4.weight _fnet.4.bias _fnet.6.weight _fnet.6.bias' + CELL_FLAT


def _pointnet(**kw):
    return pointnet.PointNet(*PRODUCTION, nfeat_global=1, **kw)


def _conv(config, bnidx):
    net = graphnet.GraphNetwork(config, 32, [13, 32, 128, 64], True, True, bnidx, 30000, use_pyg=0, cuda=1)
    return net.gconvs[0]


MODELS = {
    'pointnet': (lambda: _pointnet(nfeat_stn=2), POINTNET_ROWS, POINTNET_FLAT),
    'pointnet_nostn': (lambda: _pointnet(nfeat_stn=0), NOSTN_ROWS, NOSTN_FLAT),
    'stn': (lambda: pointnet.STNkD(2, [64, 64, 128], [128, 64]), STN_ROWS, STN_FLAT),
    'gru_bnidx2': (lambda: _conv('gru_10_0,f_13', 2), GRU_ROWS, GRU_FLAT),
    'lstm': (lambda: _conv('lstm_3_1,f_7', -1), LSTM_ROWS, LSTM_FLAT),
}


def _rows_of(module):
    return module._cfg_and_groups()[1] if isinstance(module, modules.RNNGraphConvModule) else module._groups_tensors()


def _namer(module):
    names = {id(t): n for n, t in list(module.named_parameters()) + list(module.named_buffers())}
    return lambda t: '-' if t is None else names[id(t)]


@pytest.mark.parametrize('which', sorted(MODELS))
def test_recorded_tables(which):
    """The rows of the 6-tuple table and the autograd input order are those of the parent commit, name by name."""
    build, rows_rec, flat_rec = MODELS[which]
    module = build()
    name, rows = _namer(module), _rows_of(module)
    assert all(len(r) == 6 for r in rows)
    assert [' '.join(name(t) for t in r) for r in rows] == rows_rec.strip().split('\n')
    assert [name(t) for t in _layers.flat_params(rows)] == flat_rec.split()


def test_recorded_sizes():
    """52 flat parameters of the production PointNet; n_fnet = 4, bnidx = 2, 5 rows and 16 flat parameters of the GRU module."""
    assert len(_layers.flat_params(_pointnet(nfeat_stn=2)._groups_tensors())) == 52
    conv = _conv('gru_10_0,f_13', 2)
    cfg, rows = conv._cfg_and_groups()
    assert (cfg.n_fnet, cfg.bnidx, len(rows), len(_layers.flat_params(rows))) == (4, 2, 5, 16)
    assert _conv('lstm_3_1,f_7', -1)._cfg_and_groups()[0].bnidx == -1
    assert [r.live for r in rows] == [4, 4, 4, 4, 6]


def test_tables_follow_replaced_tensors():
    """Only the structure is cached: buffers replaced by load_state_dict / .to() and re-pointed parameters show up in the next table."""
    ptn = _pointnet(nfeat_stn=2)
    before = ptn._groups_tensors()
    ptn.convs[1].running_mean = torch.ones(64)
    ptn.double()
    after = ptn._groups_tensors()
    assert after[6][4] is ptn.convs[1].running_mean and after[6][4] is not before[6][4]
    assert all(t.dtype == torch.float64 for r in after for t in r if t is not None)


# ---- gradient targets ----
def _shapes(table):
    return [[None if g is None else tuple(g.shape) for g in row] for row in table]


def test_grad_targets_batchnorm_bias_is_never_written():
    ptn = _pointnet(nfeat_stn=2)
    FlatParameters(ptn)
    rows = ptn._groups_tensors()
    tgt = _layers.grad_targets(rows)
    assert _shapes(tgt)[0] == [(64, 2, 1), None, (64,), (64,)]
    assert _shapes(tgt)[5] == [(4, 64), (4,), None, None]          # stn.proj: no norm behind it, its bias gradient is written
    assert _shapes(tgt)[-1] == [(32, 64), (32,), None, None]
    for row, trow in zip(rows, tgt):
        assert len(trow) == 4
        for k, g in enumerate(trow):
            masked = row[k] is None or (k == 1 and row[4] is not None)
            assert (g is None) == masked and (g is None or g is row[k].grad)
    assert _shapes(_layers.grad_targets(rows, strict=True)) == _shapes(tgt)


def test_grad_targets_cell_row_has_six_live_slots():
    conv = _conv('gru_10_0,f_13', 2)
    FlatParameters(conv)
    rows = conv._cfg_and_groups()[1]
    tgt = _layers.grad_targets(rows)
    assert _shapes(tgt)[2] == [(64, 128), None, (64,), (64,)]      # the filter network's BatchNorm layer
    assert _shapes(tgt)[3] == [(1024, 64), (1024,), None, None]
    assert _shapes(tgt)[4] == [(96, 32), (96, 32), (96,), (96,), (32, 32), (32,)]
    assert all(g is p.grad for g, p in zip(tgt[4], rows[4]))


@pytest.mark.parametrize('damage', ['none', 'strided'])
def test_grad_targets_missing_view(damage):
    """One .grad set to None or to a non-contiguous view: no table when lenient, the recorded message when strict."""
    ptn = _pointnet(nfeat_stn=2)
    FlatParameters(ptn)
    p = ptn.convs[3].weight
    p.grad = None if damage == 'none' else torch.zeros(64, 128, 1)[:, ::2]
    assert damage == 'none' or (p.grad.shape == p.shape and not p.grad.is_contiguous())
    rows = ptn._groups_tensors()
    assert _layers.grad_targets(rows) is None
    with pytest.raises(RuntimeError, match=r'^FusedStep: a parameter has no contiguous \.grad view into the gradient arena$'):
        _layers.grad_targets(rows, strict=True)


def test_grad_targets_groupnorm_bias_is_not_masked():
    ptn = _pointnet(nfeat_stn=0, norm='group', n_group=2)
    FlatParameters(ptn)
    rows = ptn._groups_tensors()
    assert all(r[4] is None and r[5] is None for r in rows)
    tgt = _layers.grad_targets(rows)
    assert _shapes(tgt)[0] == [(64, 14, 1), (64,), (64,), (64,)]
    assert all(trow[1] is row[1].grad for row, trow in zip(rows, tgt))


def test_arena_error_message_is_the_recorded_one():
    assert _layers.ARENA_ERROR == ('FlatParameters mode: a parameter has no contiguous .grad view into the gradient arena '
                                   '(optimizer.zero_grad(set_to_none=True) or a frozen parameter?); use FlatParameters.zero_grad()')


# ---- the cells ----
CELL_KEYS = {True: ['weight_ih', 'weight_hh', 'bias_ih', 'bias_hh', 'ig.weight', 'ig.bias'],
             False: ['weight_ih', 'weight_hh', 'bias_ih', 'bias_hh']}


@pytest.mark.parametrize('cls,base', [(modules.GRUCellEx, nn.GRUCell), (modules.LSTMCellEx, nn.LSTMCell)])
@pytest.mark.parametrize('layernorm', [True, False])
@pytest.mark.parametrize('ingate', [True, False])
def test_cell_key_order(cls, base, layernorm, ingate):
    cell = cls(32, 32, bias=True, layernorm=layernorm, ingate=ingate)
    assert isinstance(cell, base)
    assert list(cell.state_dict().keys()) == CELL_KEYS[ingate]
    assert [n for n, _ in cell.named_parameters()] == CELL_KEYS[ingate]
    assert list(cell._modules) == (['ini', 'inh'] if layernorm else []) + (['ig'] if ingate else [])
    assert repr(cell).endswith(')(' + ('ingate' if ingate else '') + (' layernorm' if layernorm else '') + ')')
    row = cell.param_tensors()
    assert row.live == 6 and len(row) == 6 and (row[4] is not None) == ingate


def test_batch_counters_advance_once_per_layer_on_host_and_module_tensors():
    ptn = _pointnet(nfeat_stn=2)
    bns = [m for m in ptn.modules() if isinstance(m, nn.BatchNorm1d)]
    assert len(bns) == 12
    ptn._bump_batches_tracked(2)
    ptn.load_state_dict(ptn.state_dict())
    bns[0].num_batches_tracked = bns[0].num_batches_tracked.clone()       # (what FlatParameters(host_counters=True) does: a new tensor)
    ptn._bump_batches_tracked(1)
    assert [int(m.num_batches_tracked) for m in bns] == [3] * 12
    fnet = _conv('gru_10_0,f_13', 2)._fnet
    _layers.advance_batch_counters(fnet)
    assert int(fnet[5].num_batches_tracked) == 1
    _layers.advance_batch_counters(_conv('lstm_3_1,f_7', -1)._fnet)      # no BatchNorm: nothing to do


# ---- what the walker refuses ----
def test_walker_refusals():
    ptn = _pointnet(nfeat_stn=0)
    ptn.convs = nn.Sequential(*(list(ptn.convs) + [nn.Sigmoid()]))
    with pytest.raises(NotImplementedError) as e:
        ptn.layer_groups()
    assert str(e.value) == 'Sigmoid is not supported by the HIP PointNet (norm must be "batch", "layer" or "group")'
    conv = _conv('gru_10_0,f_13', 2)
    conv._fnet = nn.Sequential(*(list(conv._fnet) + [nn.Dropout(0.5)]))
    with pytest.raises(NotImplementedError) as e:
        conv._cfg_and_groups()
    assert str(e.value) == 'unsupported filter-network module Dropout'
    conv = _conv('gru_10_0,f_13', 2)
    conv._fnet[5] = nn.GroupNorm(1, 128)
    with pytest.raises(NotImplementedError) as e:
        conv._cfg_and_groups()
    assert str(e.value) == 'unsupported filter-network module GroupNorm'


def test_mix_of_batchnorm_and_groupnorm_is_refused():
    ptn = _pointnet(nfeat_stn=0)
    ptn.convs[4] = nn.GroupNorm(1, 64)
    with pytest.raises(NotImplementedError) as e:
        ptn._gn_spec()
    assert str(e.value) == ('a mix of BatchNorm and GroupNorm in one model is not implemented on the HIP path '
                            '(build the STN and the PointNet with the same `norm`)')
