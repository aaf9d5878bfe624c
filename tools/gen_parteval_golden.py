"""Writes tests/golden/partition_eval.npz from the REFERENCE implementation (needs the reference checkout next to this
repository, located as tools/gen_edgeloss_golden.py does: SPG_REFERENCE; scipy): perfect_prediction (partition/provider.py), the ASA confusion matrix,
compute_OOA, compute_boundary_recall / _precision and the 2 x 2 boundary matrices (learning/metrics.py), mode,
compute_weights_SEAL and relax_edge_binary (supervized_partition/losses.py) on the two collated scenes of
tools/gen_edgeloss_golden.py with label histograms added.  Modules the reference imports and this machine may lack (plyfile,
pandas, h5py, pypcd, sklearn, libply_c) are stubbed: the functions used touch none of them.
    python tools/gen_parteval_golden.py"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import partition_eval_restatement as R  # noqa: E402
from gen_edgeloss_golden import REF, load_reference_losses, scenes  # noqa: E402

N_CLASSES, SEAL_FACTOR, TOLERANCES = 8, 5, (0, 1, 2, 3)


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return _Stub(self.__name__ + '.' + name)


def load_reference(name, *path):
    for m in ('plyfile', 'pandas', 'h5py', 'pypcd', 'sklearn', 'sklearn.neighbors', 'sklearn.decomposition'):
        try:
            importlib.import_module(m)
        except ImportError:
            sys.modules[m] = _Stub(m)
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference_function(name, *path):
    """One top-level function of a reference file, executed from the file's own text at run time.  partition/provider.py does
    not import as a module (its read_pcd has a mis-indented docstring: IndentationError), so perfect_prediction is taken
    alone: the lines from its `def` to the next line that starts in column 0."""
    lines = open(os.path.join(REF, *path)).read().split('\n')
    start = next(i for i, ln in enumerate(lines) if ln.startswith(f'def {name}('))
    end = next(i for i in range(start + 1, len(lines)) if lines[i][:1] not in ('', ' ', '\t'))
    space = {'np': np}
    exec(compile('\n'.join(lines[start:end]), os.path.join(REF, *path), 'exec'), space)
    return space[name]


def add_labels(s, rng):
    """Label histograms [n, 1 + N_CLASSES] (column 0 = unlabelled) of pruned voxels: 1-6 points of the object's class, a fifth
    of the rows mixed with a second class, 4 % of the rows unlabelled altogether, one predicted component unlabelled throughout,
    one predicted component with an exact tie between its two strongest classes; and the objects with one predicted component
    whose two most frequent objects are equally frequent."""
    obj, pred = s['objects'].copy(), s['pred_in_component'].astype(np.int64)
    n, n_com = len(obj), int(pred.max()) + 1
    cls = (obj * 5 + obj // 3) % N_CLASSES
    labels = np.zeros((n, 1 + N_CLASSES), np.uint32)
    labels[np.arange(n), 1 + cls] = rng.integers(1, 7, n)
    mixed = rng.uniform(size=n) < 0.2
    labels[mixed, 1 + (cls[mixed] + rng.integers(1, N_CLASSES, int(mixed.sum()))) % N_CLASSES] += rng.integers(1, 4, int(mixed.sum())).astype(np.uint32)
    none = rng.uniform(size=n) < 0.04
    labels[none] = 0
    labels[none, 0] = rng.integers(1, 7, int(none.sum()))
    sizes = np.bincount(pred, minlength=n_com)
    by_size = np.argsort(sizes, kind='stable')
    c_unl, c_tie, c_mode = int(by_size[0]), int(by_size[n_com // 2]), int(by_size[n_com // 2 + 1])
    rows = pred == c_unl
    labels[rows] = 0
    labels[rows, 0] = 1
    # label tie: raise the second class of c_tie to the first one's sum in one of its rows
    sums = labels[pred == c_tie, 1:].astype(np.int64).sum(0)
    a, b = np.argsort(-sums, kind='stable')[:2]
    labels[np.flatnonzero(pred == c_tie)[0], 1 + b] += np.uint32(sums[a] - sums[b])
    # mode tie: move vertices of c_mode from its most frequent object to the second one until both are equally frequent
    rows = np.flatnonzero(pred == c_mode)
    u, cnt = np.unique(obj[rows], return_counts=True)
    assert len(u) >= 2, 'the mode-tie component needs two objects'
    a, b = np.argsort(-cnt, kind='stable')[:2]
    d = int(cnt[a] - cnt[b])
    ra = rows[obj[rows] == u[a]]
    obj[ra[:d // 2]] = u[b]
    if d % 2:
        obj[ra[d // 2]] = obj.max() + 1
    return labels, obj, (c_unl, c_tie, c_mode)


def main():
    if not os.path.isdir(REF):
        sys.exit(f'reference checkout not found at {REF}')
    L = load_reference_losses()
    try:
        perfect_prediction = load_reference('ref_provider', 'partition', 'provider.py').perfect_prediction
    except IndentationError:
        perfect_prediction = load_reference_function('perfect_prediction', 'partition', 'provider.py')
    M = load_reference('ref_metrics', 'learning', 'metrics.py')
    s = scenes()
    rng = np.random.default_rng(22)
    labels, objects, (c_unl, c_tie, c_mode) = add_labels(s, rng)
    src, tgt, trans, pred = s['src'], s['tgt'], s['is_transition'], s['pred_in_component']
    n, E, n_com = len(objects), len(src), int(pred.max()) + 1
    comps = [np.flatnonzero(pred == i) for i in range(n_com)]
    out = {'src': src.astype(np.int32), 'tgt': tgt.astype(np.int32), 'is_transition': trans, 'objects': objects.astype(np.int32),
           'pred_in_component': pred.astype(np.int32), 'labels': labels, 'seal_factor': np.float64(SEAL_FACTOR)}
    # ---- majority labels ----
    per_pred = perfect_prediction(comps, labels)
    cm = M.ConfusionMatrix(N_CLASSES)
    cm.count_predicted_batch(labels[:, 1:], per_pred)
    out['full_pred'], out['confusion'] = per_pred, cm.confusion_matrix.astype(np.int64)
    assert np.array_equal(cm.confusion_matrix, out['confusion'])
    out['ooa'] = np.float64(M.compute_OOA(comps, labels))
    sums = np.stack([labels[c, 1:].astype(np.int64).sum(0) for c in comps])
    top = np.sort(sums, 1)[:, ::-1]
    label_ties = int(((top[:, 0] == top[:, 1]) & (top[:, 0] > 0)).sum())
    assert (sums[c_unl] == 0).all(), 'one component must be unlabelled throughout'
    # ---- mode, SEAL ----
    modes = [L.mode(objects[c]) for c in comps]
    out['mode_value'] = np.array([m[0] for m in modes], np.int32)
    out['mode_freq'] = np.array([m[1] for m in modes], np.int32)
    mode_ties = 0
    for c in comps:
        cnt = np.sort(np.unique(objects[c], return_counts=True)[1])[::-1]
        mode_ties += int(len(cnt) > 1 and cnt[0] == cnt[1])
    assert label_ties >= 1 and mode_ties >= 1, (label_ties, mode_ties)
    w = L.compute_weights_SEAL(comps, pred, objects, src, tgt, trans, SEAL_FACTOR)
    assert w.dtype == np.float32 and len(np.unique(w)) >= 5, np.unique(w)
    assert np.array_equal(w.view(np.uint32), R.seal_weights(src, tgt, pred, n_com, objects, trans, SEAL_FACTOR).view(np.uint32))
    out['w_seal'] = w
    # ---- relaxation, boundary recall / precision ----
    pred_trans = pred[src] != pred[tgt]
    out['pred_transition'] = pred_trans
    tolerances = []
    for tol in TOLERANCES:
        rp = L.relax_edge_binary(pred_trans, src, tgt, n, tol)
        rt = L.relax_edge_binary(trans, src, tgt, n, tol)
        grows = all(int((x != 0).sum()) < int((r != 0).sum()) < E for x, r in ((pred_trans, rp), (trans, rt)))
        if tol >= 1 and not grows:
            print(f'tolerance {tol}: the scene saturates (or does not grow); not recorded')
            break
        tolerances.append(tol)
        br, bp = M.ConfusionMatrix(2), M.ConfusionMatrix(2)
        br.count_predicted_batch_hard(trans, rp.astype('uint8'))
        bp.count_predicted_batch_hard(rt, pred_trans.astype('uint8'))
        out[f'relaxed_pred_{tol}'], out[f'relaxed_trans_{tol}'] = rp, rt
        out[f'br_counts_{tol}'], out[f'bp_counts_{tol}'] = br.confusion_matrix.astype(np.int64), bp.confusion_matrix.astype(np.int64)
        out[f'br_{tol}'] = np.float64(M.compute_boundary_recall(trans, rp))
        out[f'bp_{tol}'] = np.float64(M.compute_boundary_precision(rt, pred_trans))
        print(f'tolerance {tol}: relaxed prediction {int(rp.sum())} of {E} edges (from {int(pred_trans.sum())}), relaxed truth {int(rt.sum())} '
              f'(from {int(trans.sum())}); BR {out[f"br_{tol}"]:.4f} BP {out[f"bp_{tol}"]:.4f}; symmetric rule would give '
              f'{int(R.relax(pred_trans, src, tgt, n, tol, "symmetric").sum())} / {int(R.relax(trans, src, tgt, n, tol, "symmetric").sum())}')
    assert len(tolerances) >= 3, 'at least tolerances 0, 1, 2 must be recorded'
    out['tolerances'] = np.array(tolerances, np.int32)
    path = os.path.join(ROOT, 'tests', 'golden', 'partition_eval.npz')
    np.savez_compressed(path, **out)
    print(f'{n} vertices, {E} edges, {n_com} predicted components, {N_CLASSES} classes; components with a label tie {label_ties}, '
          f'with a mode tie {mode_ties}; unlabelled rows {int((labels[:, 1:].sum(1) == 0).sum())}, mixed rows '
          f'{int(((labels[:, 1:] > 0).sum(1) > 1).sum())}; distinct SEAL weights {len(np.unique(w))}; OOA {out["ooa"]:.4f}')
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
