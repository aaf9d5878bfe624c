"""Shared by tests/test_groupnorm_model.py and tests/test_gpu_groupnorm.py: the reference records of the GroupNorm / LayerNorm
local embedder (tools/gen_groupnorm_golden.py) and the product models that hold the recorded state."""
import functools
import os
import types

import numpy as np
import torch

from conftest import GOLDEN

ARGS = types.SimpleNamespace(ptn_nfeat_stn=2, stn_as_global=1)
CASES = [(3, 1), (5, 2), (37, 20), (130, 33)]
FILES = {'layer': 'groupnorm_embedder.npz', 'third': 'groupnorm_embedder.npz', 'group': 'groupnorm_embedder_group.npz'}


@functools.lru_cache(maxsize=None)
def golden(tag):
    return np.load(os.path.join(GOLDEN, FILES[tag]))


def state_of(tag):
    g, pre = golden(tag), f'{tag}/state/'
    return {k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)}


def cli_args(norm, n_group=2):
    """The reference CLI's defaults for the learned embeddings (supervized_partition.py:80-99)."""
    return types.SimpleNamespace(learned_embeddings=1, ptn_embedding='ptn', ver_value='ptn', ptn_nfeat_stn=2, stn_as_global=1,
                                 ptn_widths_stn=[[16, 64], [32, 16]], ptn_widths=[[32, 128], [34, 32, 32, 4]], use_rgb=1,
                                 global_feat='eXYrgb', ptn_prelast_do=0, ptn_norm=norm, ptn_n_group=n_group, cuda=0)


def build_model(tag):
    """The recorded model on the product classes (group counts as the record's: STN and PointNet alike)."""
    from superpoint_graph_amd.learning import pointnet
    nfeat, nglob, n_group = (int(v) for v in golden(tag)[f'{tag}/meta'])
    norm = str(golden(tag)[f'{tag}/norm'])
    model = torch.nn.Module()
    if tag == 'third':
        model.stn = pointnet.STNkD(2, [8, 16], [8, 4], norm=norm, n_group=n_group)
        model.ptn = pointnet.PointNet([16, 32], [16, 8, 4], [], [], nfeat, 0, prelast_do=0, nfeat_global=nglob, is_res=False, norm=norm,
                                      n_group=n_group, last_bn=True)
    else:
        model.stn = pointnet.STNkD(2, [16, 64], [32, 16], norm=norm, n_group=n_group)
        model.ptn = pointnet.PointNet([32, 128], [34, 32, 32, 4], [], [], nfeat, 0, prelast_do=0, nfeat_global=nglob, is_res=False,
                                      norm=norm, n_group=n_group, last_bn=True)
    model.load_state_dict(state_of(tag), strict=True)
    return model
