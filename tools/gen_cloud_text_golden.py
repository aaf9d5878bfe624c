"""Writes tests/golden/cloud_text.npz from the REFERENCE implementation (needs the reference checkout, located as
tools/gen_edgeloss_golden.py does: SPG_REFERENCE, and pandas + scikit-learn): read_semantic3d_format, read_s3dis_format and
interpolate_labels_batch of partition/provider.py, run as they stand on the PARITY cases of tests/cloud_text_cases.py, written
to a temporary folder.  provider.py does not compile as a whole (the indentation of read_pcd, :414-417), so the functions are
cut out of the file by name at run time and compiled on their own (none of its text is copied), with the names they use: numpy,
pandas, os, glob, NearestNeighbors and a stand-in libply_c whose prune records its arguments per chunk and hands the points
back unpruned with empty histograms (the Boost extension cannot be built here; ops.prune has its own restatement).
NearestNeighbors is wrapped to accept the positional `1` of provider.py:200, which current scikit-learn refuses, and glob.glob
returns its matches sorted, so that the order in which overlapping objects are applied is the same everywhere.
The labelled one-line case: pandas yields one empty chunk there, so prune is called once with no point.
    python tools/gen_cloud_text_golden.py"""
import glob
import os
import re
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import cloud_text_cases as C  # noqa: E402
from gen_edgeloss_golden import REF  # noqa: E402

FUNCTIONS = ('object_name_to_label', 'read_s3dis_format', 'read_semantic3d_format', 'interpolate_labels_batch')
CHUNKS = []                    # what prune received, call by call


def _prune(xyz, voxel_width, rgb, labels, objects, n_labels, n_objects):
    xyz, rgb = np.array(xyz), np.array(rgb)
    assert xyz.dtype == np.float32 and rgb.dtype == np.uint8 and xyz.flags.c_contiguous and rgb.flags.c_contiguous
    CHUNKS.append(dict(xyz=xyz, rgb=rgb, labels=np.array(labels) if n_labels > 0 else None, voxel_width=voxel_width))
    return xyz, rgb, np.zeros((len(xyz), n_labels + 1), np.uint32), np.zeros((len(xyz), n_objects + 1), np.uint32)


def load():
    with open(os.path.join(REF, 'partition', 'provider.py')) as f:
        lines = f.read().split('\n')
    import pandas as pd
    from sklearn.neighbors import NearestNeighbors
    mod = types.ModuleType('ref_provider')
    mod.__dict__.update(np=np, pd=pd, os=os, glob=glob, NearestNeighbors=NearestNeighbors,
                        libply_c=types.SimpleNamespace(prune=_prune))
    for name in FUNCTIONS:
        first = next(i for i, line in enumerate(lines) if line.startswith(f'def {name}('))
        last = next(i for i in range(first + 1, len(lines)) if re.match(r'(def|import|from|class)\b', lines[i]))
        exec(compile('\n' * first + '\n'.join(lines[first:last]), os.path.join(REF, 'partition', 'provider.py'), 'exec'), mod.__dict__)
    real = mod.NearestNeighbors

    def nearest_neighbors(*args, **kw):
        if args:
            kw['n_neighbors'] = args[0]
        return real(**kw)
    mod.NearestNeighbors = nearest_neighbors
    return mod


def write(folder, name, data):
    path = os.path.join(folder, name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'wb') as f:
        f.write(data)
    return path


def main():
    if not os.path.isdir(REF):
        sys.exit(f'reference checkout not found at {REF}')
    mod = load()
    out = {}
    real_glob = glob.glob
    glob.glob = lambda *a, **k: sorted(real_glob(*a, **k))
    try:
        with tempfile.TemporaryDirectory() as tmp:
            for name, c in C.semantic3d_cases():
                CHUNKS.clear()
                data = write(tmp, f'sema3d/{name}.txt', c['data'])
                labels = write(tmp, f'sema3d/{name}.labels', c['labels']) if c['n_class'] else ''
                res = mod.read_semantic3d_format(data, c['n_class'], labels, c['voxel_width'], c['ver_batch'])
                out[f'sema3d/{name}/n_chunks'] = np.int64(len(CHUNKS))
                for k, ch in enumerate(CHUNKS):
                    out[f'sema3d/{name}/chunk{k}/xyz'], out[f'sema3d/{name}/chunk{k}/rgb'] = ch['xyz'], ch['rgb']
                    if ch['labels'] is not None:
                        out[f'sema3d/{name}/chunk{k}/labels'] = ch['labels']
                for key, a in zip(('xyz', 'rgb', 'labels'), res):
                    out[f'sema3d/{name}/out_{key}'] = np.asarray(a)
            for name, c in C.interpolate_cases():
                data = write(tmp, f'interp/{name}.txt', c['data'])
                out[f'interp/{name}/out'] = mod.interpolate_labels_batch(data, c['xyz'], c['labels'], c['ver_batch'])
            for name, c in C.s3dis_cases():
                room = write(tmp, f's3dis/{name}/{name}.txt', c['room'])
                for fname, data in c['objects']:
                    write(tmp, f's3dis/{name}/Annotations/{fname}', data)
                for key, a in zip(('xyz', 'rgb', 'room_labels', 'room_object_indices'), mod.read_s3dis_format(room)):
                    out[f's3dis/{name}/{key}'] = a
    finally:
        glob.glob = real_glob
    path = os.path.join(ROOT, 'tests', 'golden', 'cloud_text.npz')
    np.savez_compressed(path, **out)
    for k in sorted(out):
        print(f'{k:60s} {str(out[k].dtype):8s} {out[k].shape}')
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
