"""Writes tests/golden/parsed.npz from the REFERENCE implementation (needs the reference checkout, located as
tools/gen_edgeloss_golden.py does: SPG_REFERENCE): preprocess_pointclouds of learning/s3dis_dataset.py, sema3d_dataset.py,
vkitti_dataset.py and custom_dataset.py, each run as it stands on the scenes of tests/parsed_cases.py tagged PARITY.  The four
files are loaded at run time (none of their text is copied) with stand-ins for what this machine lacks or a run must not touch:
an in-memory h5py whose files hold the arrays in the dtypes write_features / write_structure / write_spg store (a read returns a
copy, as h5py's does: the s3dis body subtracts in place), os.listdir (one scene, in the folder whose random.seed is the case's),
np.float, empty torchnet / spg modules, and the module-level `args` the sema3d function reads.  random.sample is wrapped to record
the selections.  Per case the record holds the written datasets back to back (float64; every `stride`-th row of each for the
21 000-point scene), their sizes, the centroid, the class count and the selections.
    python tools/gen_parsed_golden.py"""
import importlib.util
import os
import random
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import parsed_cases as C  # noqa: E402
from gen_edgeloss_golden import REF  # noqa: E402

FILES = {}                    # path -> {dataset name: array}: the features and superpoint-graph files of the scene
WRITTEN = {}                  # path -> {dataset name: array}: what the run wrote


class _Dataset:
    def __init__(self, a):
        self.a = a
        self.shape = a.shape

    def __getitem__(self, key):
        return np.array(self.a[key])


class _Group:
    def __init__(self, items, prefix):
        self._items, self._prefix = items, prefix

    def keys(self):
        return [k[len(self._prefix):] for k in self._items if k.startswith(self._prefix) and '/' not in k[len(self._prefix):]]


class _File:
    def __init__(self, path, mode='r'):
        self._path, self._mode = path, mode
        if mode == 'w':
            WRITTEN[path] = {}
        elif path not in FILES:
            raise OSError(f'no such file: {path}')

    def __getitem__(self, name):
        items = FILES[self._path]
        if name in items:
            return _Dataset(items[name])
        if any(k.startswith(name + '/') for k in items):
            return _Group(items, name + '/')
        raise KeyError(name)

    def create_dataset(self, name, data=None, dtype=None):
        assert self._mode == 'w'
        a = np.array(data)
        WRITTEN[self._path][name] = a if dtype is None else a.astype(dtype)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def load(dataset):
    h5 = types.ModuleType('h5py')
    h5.File = _File
    sys.modules['h5py'] = h5
    for m in ('torchnet', 'spg'):
        sys.modules[m] = types.ModuleType(m)
    if not hasattr(np, 'float'):
        np.float = float
    spec = importlib.util.spec_from_file_location(f'ref_{dataset}_dataset', os.path.join(REF, 'learning', f'{dataset}_dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    path_before = list(sys.path)
    spec.loader.exec_module(mod)
    sys.path[:] = path_before
    return mod


def folder_of(case):
    d, s = case['dataset'], case['seed']
    return {'s3dis': f'Area_{s:d}', 'vkitti': f'0{s:d}'}.get(d, 'train')


def run(mod, case, root):
    """-> (the written datasets {name: array}, class_count or None, the selections in the order they were drawn)"""
    FILES.clear(), WRITTEN.clear()
    d, folder = case['dataset'], folder_of(case)
    feat = 'features_supervision' if d == 'vkitti' or (d == 's3dis' and case['supervized_partition']) else 'features'
    pathD, pathC, pathP = (f'{root}/{k}/{folder}/' for k in (feat, 'superpoint_graphs', 'parsed'))
    g = case['geof']
    FILES[pathD + 'scene.h5'] = dict(xyz=case['xyz'], rgb=case['rgb'], labels=case['labels'], geof=g, elevation=case['elevation'],
                                     linearity=g[:, 0], planarity=g[:, 1], scattering=g[:, 2], verticality=g[:, 3])
    FILES[pathC + 'scene.h5'] = {f'components/{c:d}': np.asarray(idx, dtype=np.uint32) for c, idx in enumerate(case['components'])}
    drawn = []
    real_listdir, real_sample = os.listdir, random.sample

    def listdir(path):
        return ['scene.h5'] if path == pathC else ([] if path.startswith(root) else real_listdir(path))

    def sample(population, k):
        r = real_sample(population, k=k)
        drawn.append(np.asarray(r, dtype=np.int32))
        return r
    os.listdir, random.sample = listdir, sample
    try:
        if d == 's3dis':
            mod.preprocess_pointclouds(types.SimpleNamespace(S3DIS_PATH=root, supervized_partition=case['supervized_partition'],
                                                             plane_model_elevation=case['plane_model_elevation']))
        else:
            mod.args = types.SimpleNamespace(supervised_partition=0)
            mod.preprocess_pointclouds(root)
    finally:
        os.listdir, random.sample = real_listdir, real_sample
    count = WRITTEN.get(f'{root}/parsed/class_count.h5', {}).get('class_count')
    if count is not None and count.ndim == 2:
        assert not np.delete(count, case['seed'] - 1, axis=1).any()
        count = count[:, case['seed'] - 1]
    return WRITTEN[pathP + 'scene.h5'], count, drawn


def main():
    if not os.path.isdir(REF):
        sys.exit(f'reference checkout not found at {REF}')
    mods = {d: load(d) for d in ('s3dis', 'sema3d', 'vkitti', 'custom')}
    out = {}
    for case in C.cases():
        if 'PARITY' not in case['tags']:
            continue
        assert case['max_points'] == 10000 and not (case['plane_model_elevation'] and not case['supervized_partition'])
        with tempfile.TemporaryDirectory() as root, np.errstate(all='ignore'):
            written, count, drawn = run(mods[case['dataset']], case, root)
        name, C_ = case['name'], len(case['components'])
        data = [written[f'{c:d}'] for c in range(C_)]
        assert len(written) == C_ + (case['dataset'] != 'custom')
        out[f'{name}/sizes'] = np.array([len(a) for a in data], np.int64)
        out[f'{name}/rows'] = np.concatenate([a[::case['stride']] for a in data], 0)
        assert out[f'{name}/rows'].dtype == np.float64
        if case['dataset'] != 'custom':
            out[f'{name}/centroid'] = written['centroid']
            out[f'{name}/class_count'] = np.asarray(count, np.int64)
        big = [c for c in range(C_) if len(case['components'][c]) > 10000]
        assert len(big) == len(drawn)
        for c, sel in zip(big, drawn):
            out[f'{name}/trim{c:d}'] = sel
    assert any(k.split('/')[1].startswith('trim') for k in out), 'no trimmed component in the record'
    path = os.path.join(ROOT, 'tests', 'golden', 'parsed.npz')
    np.savez_compressed(path, **out)
    print(len({k.split('/')[0] for k in out}), 'cases;', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
