"""CPU, skipped when the reference checkout is absent (SPG_REFERENCE names it): `create_model` of this package at the superpoint
embedding widths 16 and 64 (--ptn_widths "[[64,64,128,128,256],[256,64,W]]": W is the state width of the recurrent cell and of the
edge filters) builds what the reference's own learning/main.py builds out of the reference's own modules -- the same state_dict
keys and shapes, and under the same seed bit-identical parameters -- so that a checkpoint trained with such a width loads here."""
import argparse
import os
import sys
import types

import pytest
import torch

REF = os.environ.get('SPG_REFERENCE', '/root/reference')
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'learning')), reason='reference checkout not present')


@pytest.fixture()
def ref_main():
    """The reference's learning.main with the reference's own pointnet / graphnet / modules (no aliasing)."""
    saved, saved_path = dict(sys.modules), list(sys.path)
    try:
        # loader-side dependencies that are not installed offline and are irrelevant to model creation
        for name in ('h5py', 'igraph', 'torchnet', 'transforms3d', 'transforms3d.zooms', 'transforms3d.axangles'):
            if name not in sys.modules:
                sys.modules[name] = types.ModuleType(name)
        for k in [k for k in sys.modules if k == 'learning' or k.startswith('learning.') or k == 'ecc']:
            del sys.modules[k]
        sys.path.insert(0, REF)
        from learning import main as ref_main_mod
        assert os.path.abspath(ref_main_mod.graphnet.__file__).startswith(os.path.abspath(REF))
        yield ref_main_mod
    finally:
        sys.path[:] = saved_path
        for k in list(sys.modules):
            if k not in saved:
                del sys.modules[k]
        sys.modules.update(saved)


def _args(width, model_config):
    return argparse.Namespace(model_config=model_config, ptn_widths=[[64, 64, 128, 128, 256], [256, 64, width]],
                              ptn_widths_stn=[[64, 64, 128], [128, 64]], ptn_nfeat_stn=14, ptn_prelast_do=0,
                              fnet_widths=[32, 128, 64], fnet_orthoinit=1, fnet_llbias=0, fnet_bnidx=2,
                              edge_mem_limit=30000, use_pyg=0, cuda=0)


@pytest.mark.parametrize('width,model_config', [(16, 'gru_10_1,f_13'), (16, 'lstm_3_0_1_1_0,f_13'), (64, 'gru_10_0,f_13'), (64, 'lstm_4_1,f_13')])
def test_create_model_matches_the_reference(ref_main, width, model_config, capsys):
    from superpoint_graph_amd.learning import graphnet, main as amd_main
    dbinfo = dict(node_feats=14, edge_feats=13, classes=13)
    ref_main.set_seed(3, cuda=False)
    ref = ref_main.create_model(_args(width, model_config), dbinfo)
    amd_main.set_seed(3, cuda=False)
    ours = amd_main.create_model(_args(width, model_config), dbinfo)
    capsys.readouterr()                              # (the reference prints the model)
    assert isinstance(ours.ecc, graphnet.GraphNetwork) and not isinstance(ref.ecc, graphnet.GraphNetwork)
    cell = ours.ecc.gconvs[0]._cell
    assert cell.hidden_size == width and cell.input_size == width
    sd_ref, sd = ref.state_dict(), ours.state_dict()
    assert list(sd.keys()) == list(sd_ref.keys())
    for k, v in sd_ref.items():
        assert sd[k].shape == v.shape and sd[k].dtype == v.dtype, k
        assert torch.equal(sd[k], v), k
    gates = 4 if model_config.startswith('lstm') else 3
    assert sd['ecc.0._cell.weight_ih'].shape == (gates * width, width) and sd['ecc.0._cell.ig.weight'].shape == (width, width)
    nout = width if model_config.split(',')[0].split('_')[2] == '1' else width * width
    assert sd['ecc.0._fnet.7.weight'].shape == (nout, 64)
