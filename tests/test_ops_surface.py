"""The surface of superpoint_graph_amd.ops and the import graph of its modules, on the host (importing ops needs torch, not the built
library).  SURFACE was recorded once from the single-file ops module that the package replaced: every public name defined there with its
kind, str(inspect.signature(...)) of callables, the sorted public methods of classes and the value of constants."""
import ast
import inspect
import os
import sys

SURFACE = {'CLASS_COUNT_MAX': ('constant', 4096),
 'CP_MAX_D': ('constant', 32),
 'CloudTextError': ('class', "(line, code, offset, refused, source='')", []),
 'CloudTextReader': ('class',
                     '(path, n_cols, xyz_cols=(0, 1, 2), rgb_cols=None, label_col=None, rows=1048576, block_bytes=67108864, skip_lines=0, '
                     'device=None)',
                     []),
 'DeviceGraph': ('class', "(idxn: 'torch.Tensor', degs: 'torch.Tensor', n_src: 'Optional[int]' = None)", ['export', 'from_workspace']),
 'EDGE_MAX_D': ('constant', 64),
 'EccRnnState': ('class', '(cfg, graph, edgefeats, ws, training)', []),
 'EdgeGraph': ('class', "(src, tgt, n: 'int')", ['build']),
 'GroupNormState': ('class', '(cfg, B, clouds, clouds_global, ws, ext_transform)', []),
 'KNN_MAX_K': ('constant', 47),
 'KnnIndex': ('class', "(ref_xyz, cell_size=None, query_capacity: 'int' = 0)", ['query', 'query_chunk', 'self_query']),
 'MINCUT_LIMIT': ('constant', 268435456),
 'MINCUT_MAX_PULSES': ('constant', 65536),
 'PARSED_RECIPES': ('constant', {'custom': (1, 11), 's3dis': (0, 15), 'sema3d': (1, 11), 'vkitti': (2, 14)}),
 'PARTEVAL_MAX_CLASSES': ('constant', 64),
 'PLANE_MAX_TRIALS': ('constant', 1024),
 'PartitionIndex': ('class', "(in_component, n_com: 'int', _flag=None)", []),
 'PointNetState': ('class', '(cfg, B, clouds, clouds_global, ws, training, ext_transform=None)', []),
 'ResidentSPG': ('class', "(edges, feats, sizes, n: 'int')", []),
 'SPGSample': ('class', '()', []),
 'TEXT_ERRORS': ('constant',
                 {1: 'the wrong number of fields',
                  2: 'an empty field (a leading, trailing or double space)',
                  3: 'a byte that is not part of a number',
                  4: 'a field outside the number grammar ([+-]digits[.digits], at most 15 digits, at most 22 behind the point, no exponent)',
                  5: 'a colour or label that is not a whole number in [0, 255]',
                  6: 'a line longer than the cap'}),
 'TEXT_MAX_COLS': ('constant', 16),
 'TILES_MAX_K': ('constant', 64),
 'TILES_VERTICES_PER_BLOCK': ('constant', 32),
 'augment_whole': ('function', '(xyz, rgb, ref_point=None, M=None, noise_xyz=None, noise_rgb=None)'),
 'batch_graph_build': ('function', "(edges_h: 'torch.Tensor', feats_h: 'Optional[torch.Tensor]', n_nodes: 'int', device=None)"),
 'batch_graph_fits': ('function', "(n_nodes: 'int', n_edges: 'int', n_feat: 'int') -> 'bool'"),
 'boundary_counts': ('function', '(a, b)'),
 'check_persistent_ecc': ('function', "(what='training', group=None)"),
 'class_count': ('function', "(labels, n_classes: 'int')"),
 'colsum': ('function', '(x, out=None)'),
 'component_label_majority': ('function', "(index: 'PartitionIndex', labels)"),
 'component_mode': ('function', "(index: 'PartitionIndex', values)"),
 'compute_geof': ('function', "(xyz, target, k_nn: 'int')"),
 'connected_components': ('function', "(graph: 'EdgeGraph', active)"),
 'contrastive_edge_loss': ('function', "(embeddings, graph: 'EdgeGraph', is_transition, weights, loss='TVH_zhang', dist_type='euclidian')"),
 'cross_entropy': ('function', "(logits, target, weight=None, ignore_index=-100, reduction='mean', return_normaliser=False)"),
 'crosspartition_weights': ('function', "(graph: 'EdgeGraph', pred_in_component, is_transition, factor, return_components=False)"),
 'cut_pursuit': ('function',
                 "(obs, graph: 'EdgeGraph', edge_weight, node_weight=None, reg_strength=None, cutoff: 'int' = 0, weight_decay: 'float' = 1.0, "
                 "max_ite: 'int' = 5, kmeans_ite: 'int' = 3, flow_steps: 'int' = 2, max_pulses: 'Optional[int]' = None, return_stats: 'bool' = "
                 'False)'),
 'ecc_aggregate_bwd': ('function', "(x, w, grad_out, graph: 'DeviceGraph', idxe=None, need_x=True, need_w=True)"),
 'ecc_aggregate_fwd': ('function', "(x, w, graph: 'DeviceGraph', idxe=None, cin=None, cout=None)"),
 'eccrnn_backward': ('function', "(state: 'EccRnnState', groups, grad_out, out_grads=None)"),
 'eccrnn_forward': ('function', "(cfg: 'EccRnnCfg', graph: 'DeviceGraph', h0, edgefeats, groups, training: 'bool', bn_update_times: 'int' = 1)"),
 'edge_dist': ('function', "(embeddings, graph: 'EdgeGraph', dist_type='euclidian')"),
 'edge_features': ('function', '(columns, edges, mean=None, scale=None)'),
 'edge_loss': ('function', "(diff, is_transition, weights, loss='TVH_zhang', dist_type='euclidian')"),
 'eval_accumulate': ('function', '(logits, label_mode, label_vec, confusion, counters)'),
 'gather_rows': ('function', '(src, perm)'),
 'gn_backward': ('function', "(state: 'GroupNormState', groups, grad_emb, want_clouds=False)"),
 'gn_forward': ('function', "(cfg: 'GnCfg', clouds, clouds_global, groups, ext_transform=None)"),
 'gru_cell_bwd': ('function', "(inp, hidden, grad_out, params, layernorm: 'bool', ingate: 'bool')"),
 'gru_cell_fwd': ('function', "(inp, hidden, params: 'Sequence[Optional[torch.Tensor]]', layernorm: 'bool', ingate: 'bool')"),
 'induced_subgraph': ('function', "(graph: 'EdgeGraph', selected_ver, selected_edg)"),
 'knn': ('function', "(ref_xyz, k: 'int', query_xyz=None, cell_size=None, distances: 'bool' = True)"),
 'linear_backward': ('function', '(dy, x, w, need_dx=True, has_bias=True, out_w=None, out_b=None)'),
 'linear_dgrad': ('function', '(dy, w)'),
 'linear_fwd': ('function', '(x, w, bias=None, in_scale=None, in_shift=None, in_relu=False)'),
 'linear_wgrad': ('function', '(dy, x, in_scale=None, in_shift=None, in_relu=False, out=None)'),
 'linear_wgrad_bias': ('function', '(dy, x, out_w=None, out_b=None)'),
 'load_superpoints': ('function', "(points, offsets, slot, sample_idx, colmap, xyznormalize: 'bool', n_valid: 'int', M=None, noise=None)"),
 'loader_random': ('function',
                   "(counts, ids, slot, npts: 'int', nfeat: 'int', n_valid: 'int', seed: 'int', step: 'int', augment: 'bool', scale: 'float' = 0.0, "
                   "rot: 'bool' = False, mirror_prob: 'float' = 0.0, jitter: 'bool' = False)"),
 'lstm_cell_bwd': ('function', "(inp, h, c, grad_hy, grad_cy, params, layernorm: 'bool', ingate: 'bool')"),
 'lstm_cell_fwd': ('function', "(inp, h, c, params: 'Sequence[Optional[torch.Tensor]]', layernorm: 'bool', ingate: 'bool')"),
 'make_eccrnn_cfg': ('function',
                     "(nc, nrepeats, matrix, layernorm, ingate, cat_all, fnet_widths, bnidx, llbias, bn_eps=1e-05, bn_momentum=0.1, cell='gru') -> "
                     "'EccRnnCfg'"),
 'make_gn_cfg': ('function', "(nfeat, nfeat_global, npts, conv, fc, n_group, eps=1e-05, last_ac=False) -> 'GnCfg'"),
 'make_pointnet_cfg': ('function',
                       '(nfeat, nfeat_stn, nfeat_global, npts, stn_conv, stn_fc, conv, fc, last_ac=False, bn_eps=1e-05, bn_momentum=0.1) -> '
                       "'PointNetCfg'"),
 'min_cut': ('function', "(graph: 'EdgeGraph', cap, cost0, cost1, max_pulses: 'Optional[int]' = None, return_info: 'bool' = False)"),
 'neighbourhood_tiles': ('function',
                         "(xyz, nei, k: 'int', rows=None, rgb=None, global_feat='', elevation=None, xyn=None, cloud_rgb=True, stream_stores=True)"),
 'parse_cloud_text': ('function',
                      "(text_u8, n_cols, xyz_cols=(0, 1, 2), rgb_cols=None, label_col=None, final_block=True, line_base=0, byte_base=0, source='')"),
 'parsed_points': ('function', "(recipe, xyz, rgb, comp_off, comp_idx, geof=None, elevation=None, trim=None, lpsv_raw: 'bool' = False)"),
 'partition_scores': ('function', "(graph: 'EdgeGraph', pred_in_component, n_com: 'int', is_transition, labels, tolerance: 'int')"),
 'persistent_ecc_status': ('function', '(clear=False)'),
 'plane_elevation': ('function', "(xyz, subsets=None, seed: 'int' = 0, max_trials: 'int' = 100, low_height: 'float' = 0.5)"),
 'pointnet_backward': ('function', "(state: 'PointNetState', groups, grad_emb, out_grads=None, want_input_grads=False)"),
 'pointnet_forward': ('function',
                      "(cfg: 'PointNetCfg', clouds, clouds_global, groups: 'List[Sequence[Optional[torch.Tensor]]]', training: 'bool', "
                      "bn_update_times: 'int' = 1, ext_transform=None)"),
 'prune': ('function', "(xyz, voxel_size: 'float', rgb=None, labels=None, objects=None, n_labels: 'int' = 0, n_objects: 'int' = 0)"),
 'random_subgraph': ('function', "(graph: 'EdgeGraph', subgraph_size: 'int', seeds, state=None)"),
 'ransac_subsets': ('function', "(n_low: 'int', trials: 'int' = 100, seed: 'int' = 0)"),
 'recover_persistent_ecc': ('function', '(arena=None, group=None)'),
 'relax_edges': ('function', "(graph: 'EdgeGraph', binary, tolerance: 'int', mode='reference')"),
 'sample_spg': ('function', "(g: 'ResidentSPG', perm=None, centres=None, order: 'int' = 0, minpts: 'int' = 0, hardcutoff: 'int' = 0) -> 'SPGSample'"),
 'scene_stats': ('function', "(xyz, with_distance: 'bool' = False)"),
 'scene_structure': ('function', "(xyz, knn_idx, k_adj: 'int', ids=None, hist=None, id_mode='objects', geof=None, rgb=None)"),
 'seal_weights': ('function', "(graph: 'EdgeGraph', index: 'PartitionIndex', objects, is_transition, factor)"),
 'set_batch': ('function', "(edges, n_nodes: 'int')"),
 'sp_graph': ('function', "(xyz, comp, n_com: 'int', tets, d_max: 'float', labels=None, label_rows=None, n_labels: 'int' = 0)"),
 'text_layout': ('function', '()'),
 'upload': ('function', "(host: 'torch.Tensor', device=None) -> 'torch.Tensor'"),
 'upload_packed': ('function', '(hosts, device=None)')}

# what else `ops.NAME` has to resolve: the library handle and the private helpers that tests and tools reach through the package
EXTRA = {'check', 'lib', '_lib', '_stream', '_ptr', '_req', '_ptr_array', '_loss_codes', '_text_roles', '_edge_forward', '_component_mode',
         '_relax', '_cp_sums', '_cp_dist', '_cp_farthest'}

# module -> the modules of the package it may import (every one of them may import _core)
MAY_IMPORT = {'_core': set(), 'model': set(), 'batch': {'model'}, 'spgraph': set(), 'edges': set(), 'text': set(), 'parteval': {'edges'},
              'tiles': {'edges'}, 'sample': {'edges'}, 'scene': {'edges', 'spgraph', 'parteval'}, 'cutpursuit': {'edges'}}


def _describe(name, obj):
    if inspect.isclass(obj):
        return ('class', str(inspect.signature(obj)), sorted(m for m in vars(obj) if not m.startswith('_') and callable(getattr(obj, m))))
    if inspect.isfunction(obj):
        return ('function', str(inspect.signature(obj)))
    return ('constant', obj)


def test_ops_surface_is_the_recorded_one():
    from superpoint_graph_amd import ops
    assert len(SURFACE) == 89
    exposed = {n for n, o in vars(ops).items() if not inspect.ismodule(o) and not (n.startswith('__') and n.endswith('__'))}
    modules = {n for n, o in vars(ops).items() if inspect.ismodule(o)}
    assert exposed | {'_lib'} == set(SURFACE) | EXTRA, sorted(exposed ^ (set(SURFACE) | EXTRA))
    assert modules == set(MAY_IMPORT) | {'_lib'}                                # nothing public besides the stage modules themselves
    assert all(hasattr(ops, n) for n in EXTRA)
    for name, recorded in SURFACE.items():
        assert _describe(name, getattr(ops, name)) == recorded, name


def test_ops_import_graph():
    from superpoint_graph_amd import ops
    root = os.path.dirname(ops.__file__)
    files = sorted(f[:-3] for f in os.listdir(root) if f.endswith('.py'))
    assert files == sorted(list(MAY_IMPORT) + ['__init__'])
    for mod in files:
        with open(os.path.join(root, mod + '.py')) as f:
            tree = ast.parse(f.read())
        imports = [n for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))]
        assert all(n in tree.body for n in imports), f'{mod}: an import inside a function or class body'
        if mod == '__init__':                                                       # a docstring and imports, nothing else
            assert all(isinstance(n, ast.ImportFrom) or n is tree.body[0] and isinstance(n, ast.Expr) for n in tree.body)
            continue
        for n in imports:
            if isinstance(n, ast.Import):
                tops = {a.name.split('.')[0] for a in n.names}
            elif n.level == 0:
                tops = {n.module.split('.')[0]}
            else:
                tops = set()
                if n.level == 2:                                                    # the parent package: its ctypes loader only
                    assert (n.module or n.names[0].name) == '_lib' and (n.module or len(n.names) == 1), f'{mod}: {ast.dump(n)}'
                else:                                                               # a sibling, by name (never `from . import`: the root)
                    assert n.level == 1 and n.module in MAY_IMPORT[mod] | {'_core'}, f'{mod} imports {n.module}'
            assert 'superpoint_graph_amd' not in tops, f'{mod}: absolute import of the package'
            if mod == '_core':
                assert all(t in ('torch', 'numpy') or t in sys.stdlib_module_names for t in tops), f'_core imports {tops}'
