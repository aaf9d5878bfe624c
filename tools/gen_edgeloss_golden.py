"""Writes tests/golden/edge_loss.npz from the REFERENCE implementation (needs the reference checkout next to this repository:
SPG_REFERENCE or /root/reference, scipy): compute_dist, compute_loss, their backward, compute_weights_XPART and the
'proportional' weights of supervized_partition/losses.py on two collated synthetic scenes.  The module imports once
`partition`, `partition.provider`, `partition.ply_c` (+ `.libply_c`) and `libcp` are stubbed; the libply_c.connected_comp stub
uses scipy.sparse.csgraph.connected_components (only the component membership enters the weights).
    python tools/gen_edgeloss_golden.py"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('SPG_REFERENCE', '/root/reference')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import edge_loss_restatement as R  # noqa: E402

K_NN_ADJ, TRANSITION_FACTOR = 5, 5
LOSSES = ['tv_zhang', 'tv_TVminus', 'laplacian_zhang', 'laplacian_TVminus', 'TVH_zhang', 'TVH_TVminus']
CASES = [(name, 'euclidian') for name in LOSSES] + [('TVH_zhang', 'intrinsic'), ('TVH_zhang', 'scalar')]
RTOL, ATOL_FRAC = 1e-4, 1e-5                      # the project bound (tests/conftest.py assert_elementwise)


def connected_comp(n_ver, source, target, active, cutoff):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    assert cutoff == 0
    keep = np.asarray(active) != 0
    adj = coo_matrix((np.ones(int(keep.sum())), (source[keep].astype(np.int64), target[keep].astype(np.int64))), shape=(n_ver, n_ver))
    k, lab = connected_components(adj, directed=False)
    return [np.flatnonzero(lab == i) for i in range(k)], lab.astype(np.uint32)


def load_reference_losses():
    for name in ('partition', 'partition.provider', 'partition.ply_c', 'partition.ply_c.libply_c', 'libcp'):
        sys.modules[name] = types.ModuleType(name)
    sys.modules['partition.ply_c'].libply_c = sys.modules['partition.ply_c.libply_c']
    sys.modules['partition.ply_c.libply_c'].connected_comp = connected_comp
    spec = importlib.util.spec_from_file_location('ref_losses', os.path.join(REF, 'supervized_partition', 'losses.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scenes():
    """Two collated scenes: positions, a k_nn_adj nearest-neighbour adjacency, objects from spatial bins, a coarser predicted
    partition from shifted bins, 1 % of the remaining edges marked as transitions too (so that some transition edges have both
    ends in one cross component), unit embeddings around one centre per object."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(21)
    src, tgt, obj, pred, xyz = [], [], [], [], []
    off = 0
    for n in (1500, 1450):
        p = rng.uniform(0, 4, size=(n, 3)).astype(np.float32) * np.float32([1, 1, 0.25])
        _, nb = cKDTree(p).query(p, K_NN_ADJ + 1)
        src.append(np.repeat(np.arange(n), K_NN_ADJ) + off)
        tgt.append(nb[:, 1:].reshape(-1) + off)
        obj.append((np.floor(p[:, 0]) * 4 + np.floor(p[:, 1])).astype(np.int64) + 16 * len(obj))
        pred.append((np.floor((p[:, 0] + 0.7) / 2) * 4 + np.floor((p[:, 1] + 0.3) / 2)).astype(np.int64) + 16 * len(pred))
        xyz.append(p)
        off += n
    src, tgt, obj = np.concatenate(src), np.concatenate(tgt), np.concatenate(obj)
    pred = np.unique(np.concatenate(pred), return_inverse=True)[1].astype(np.uint32)
    trans = (obj[src] != obj[tgt])
    trans |= (~trans) & (rng.uniform(size=len(src)) < 0.01)
    centres = rng.normal(size=(int(obj.max()) + 1, 4))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    n = off
    emb = np.zeros((n, 4), np.float32)
    todo = np.arange(n)
    for _ in range(200):                                # |<e_s, e_t>| <= 0.98 on every edge: redraw the sources of the others
        e = centres[obj[todo]] + 0.6 * rng.normal(size=(len(todo), 4))
        emb[todo] = (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)
        dot = (emb[src].astype(np.float64) * emb[tgt].astype(np.float64)).sum(1)
        todo = np.unique(src[np.abs(dot) > 0.975])
        if len(todo) == 0:
            break
    emb = (emb.astype(np.float64) / np.linalg.norm(emb.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return dict(emb=emb, src=src.astype(np.int64), tgt=tgt.astype(np.int64), is_transition=trans.astype(np.uint8),
                objects=obj, pred_in_component=pred, xyz=np.concatenate(xyz))


def within(a, ref, frac, what):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(a), nan), f'{what}: NaN pattern differs'
    bound = frac * (RTOL * np.abs(ref) + ATOL_FRAC * np.nanmax(np.abs(ref)) if (~nan).any() else 0.0)
    worst = np.max(np.where(nan, 0.0, np.abs(a - ref) - bound)) if a.size else 0.0
    assert worst <= 0.0, f'{what}: the reference is further than {frac} x the project bound from float64 (by {worst:.3e})'


def main():
    if not os.path.isdir(REF):
        sys.exit(f'reference checkout not found at {REF}')
    torch.manual_seed(0)
    L = load_reference_losses()
    s = scenes()
    src, tgt, trans = s['src'], s['tgt'], s['is_transition']
    n, E = len(s['emb']), len(src)
    dot = (s['emb'][src].astype(np.float64) * s['emb'][tgt].astype(np.float64)).sum(1)
    assert np.abs(dot).max() <= 0.98, np.abs(dot).max()
    out = {'emb': s['emb'], 'src': src.astype(np.int32), 'tgt': tgt.astype(np.int32), 'is_transition': trans,
           'objects': s['objects'].astype(np.int32), 'pred_in_component': s['pred_in_component']}
    # ---- weights ----
    factor = TRANSITION_FACTOR * 2 * K_NN_ADJ
    pred_components = [np.flatnonzero(s['pred_in_component'] == i) for i in range(int(s['pred_in_component'].max()) + 1)]
    w_x = L.compute_weights_XPART(pred_components, s['pred_in_component'], s['objects'], src, tgt, trans, factor, s['xyz'])
    w_r, comp_r, size_r = R.xpart_weights(n, src, tgt, trans, s['pred_in_component'], factor)
    assert w_x.dtype == np.float32 and np.array_equal(w_x.view(np.uint32), w_r.view(np.uint32)), 'closed form is not bit-equal to the loop'
    same = comp_r[src] == comp_r[tgt]
    assert (trans != 0).sum() > 100 and (same & (trans != 0)).sum() > 5, 'no transition edge inside one cross component'
    pt = s['pred_in_component'][src] != s['pred_in_component'][tgt]
    assert (pt & (trans == 0)).sum() > 50 and (~pt & (trans != 0)).sum() > 50, 'both kinds of boundary must occur'
    args = types.SimpleNamespace(loss_weight='proportional', transition_factor=TRANSITION_FACTOR, k_nn_adj=K_NN_ADJ, cuda=0)
    w_p = L.compute_weight_loss(args, torch.from_numpy(s['emb']), torch.from_numpy(s['objects']), src, tgt, torch.from_numpy(trans), None, False)
    out['w_xpart'], out['w_proportional'] = w_x, w_p.numpy().astype(np.float32)
    out['xpart_factor'] = np.float64(factor)
    out['transition_factor'] = np.float64(TRANSITION_FACTOR)
    # ---- distance, loss, gradient ----
    weights = torch.from_numpy(w_x)
    for dist_type in ('euclidian', 'intrinsic', 'scalar'):
        diff = L.compute_dist(torch.from_numpy(s['emb']), src, tgt, dist_type).numpy()
        within(diff, R.dist(s['emb'], src, tgt, dist_type)[0], 0.25, f'diff {dist_type}')
        out[f'diff_{dist_type}'] = diff
    for name, dist_type in CASES:
        emb = torch.from_numpy(s['emb']).clone().requires_grad_(True)
        a = types.SimpleNamespace(loss=name, dist_type=dist_type)
        diff = L.compute_dist(emb, src, tgt, dist_type)
        l1, l2 = L.compute_loss(a, diff, torch.from_numpy(trans), weights)
        ((l1 + l2) / E * 1000).backward()
        _, r1, r2, rg = R.loss_and_grad(s['emb'], src, tgt, trans, w_x, name, dist_type, 1000.0 / E)
        for v, r, what in ((l1.item(), r1, 'loss1'), (l2.item(), r2, 'loss2')):
            assert (np.isnan(v) and np.isnan(r)) or abs(v - r) <= 0.25 * (RTOL + ATOL_FRAC) * abs(r), (name, dist_type, what, v, r)
        within(emb.grad.numpy(), rg, 0.25, f'gradient {name} {dist_type}')
        out[f'{name}_{dist_type}_loss'] = np.array([l1.item(), l2.item()], np.float32)
        out[f'{name}_{dist_type}_grad'] = emb.grad.numpy()
        print(f'{name:18s} {dist_type:10s} loss1 {l1.item():.6g} loss2 {l2.item():.6g} max|grad| {np.nanmax(np.abs(emb.grad.numpy())) if not np.isnan(emb.grad.numpy()).all() else float("nan"):.4g}'
              f' NaN grads {int(np.isnan(emb.grad.numpy()).sum())}')
    path = os.path.join(ROOT, 'tests', 'golden', 'edge_loss.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', n, 'vertices,', E, 'edges,', int((trans != 0).sum()), 'transitions')


if __name__ == '__main__':
    main()
