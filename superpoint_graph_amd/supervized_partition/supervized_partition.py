"""Model construction of the learned partition (reference supervized_partition/supervized_partition.py:411-434).

`create_model(args)` builds what the reference's training script builds for the learned embeddings: a stand-alone spatial
transformer `model.stn` and a PointNet without inner transformer `model.ptn`, evaluated together by
`learning.pointnet.LocalCloudEmbedder`.  The two flags that reach only this embedder are honoured: `ptn_norm`
('batch' | 'layer' | 'group') and `ptn_n_group`; module order and state_dict keys are the reference's, so its checkpoints load
with strict=True.  For the hand-crafted vertex values (ver_value 'geof' / 'geofrgb', learned_embeddings 0: :423-428) the model is
the reference's single placeholder parameter.  The training loop itself is not part of this package; what it calls per step is
(losses.py, and cut pursuit through compute_weight_loss(..., partition='device'))."""
import torch
import torch.nn as nn

from ..learning.pointnet import PointNet, STNkD


def create_model(args):
    """-> nn.Module with .stn (if ptn_nfeat_stn > 0) and .ptn for the learned embeddings (ver_value 'ptn'), or with .placeholder
    alone for ver_value 'geof' / 'geofrgb' (learned_embeddings 0, as the reference's parser derives it from ver_value)."""
    if getattr(args, 'ver_value', 'ptn') in ('geof', 'geofrgb'):
        if args.learned_embeddings:
            raise NotImplementedError(f"create_model: ver_value {args.ver_value!r} goes with learned_embeddings 0 (the reference's parser sets "
                                      "learned_embeddings = 'ptn' in ver_value or ver_value == 'xyz'); the geof values with a learned "
                                      "embedder are not a model the reference trains")
        model = nn.Module()
        model.placeholder = nn.Parameter(torch.tensor(0.0))
        if getattr(args, 'cuda', 0):
            model.cuda()
        return model
    if not args.learned_embeddings or 'ptn' not in args.ptn_embedding:
        raise NotImplementedError("create_model: only the learned embeddings (learned_embeddings = 1, ptn_embedding 'ptn') are built")
    norm, n_group = getattr(args, 'ptn_norm', 'batch'), getattr(args, 'ptn_n_group', 2)
    model = nn.Module()
    if args.ptn_nfeat_stn > 0:
        model.stn = STNkD(args.ptn_nfeat_stn, args.ptn_widths_stn[0], args.ptn_widths_stn[1], norm=norm, n_group=n_group)
    n_feat = 3 + 3 * args.use_rgb
    nfeats_global = len(args.global_feat) + 4 * args.stn_as_global + 1      # the diameter is always there
    # (the reference does not hand n_group to the PointNet: with ptn_norm 'group' its layers get the class default)
    model.ptn = PointNet(args.ptn_widths[0], args.ptn_widths[1], [], [], n_feat, 0, prelast_do=args.ptn_prelast_do,
                         nfeat_global=nfeats_global, norm=norm, is_res=False, last_bn=True)
    if getattr(args, 'cuda', 0):
        model.cuda()
    return model
