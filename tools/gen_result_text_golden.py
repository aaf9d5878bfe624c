"""Writes tests/golden/result_text.npz from the REFERENCE implementation (needs the reference checkout, located as
tools/gen_edgeloss_golden.py does: SPG_REFERENCE): the nine ASCII PLY writers of partition/provider.py (write_ply,
write_ply_labels, write_ply_obj, partition2ply, geof2ply, prediction2ply, error2ply, spg2ply, scalar2ply) and
get_color_from_label, run as they stand on the inputs of tests/result_text_cases.py.  provider.py does not compile as a whole
(the indentation of read_pcd), so the functions are cut out of the file by name at run time and compiled on their own (none of
its text is copied), with the names they use: numpy, random, colorsys and stand-ins for plyfile's PlyElement.describe and
PlyData(..., text=True).write, which capture the structured arrays, the element names and the text flag instead of writing
(plyfile is not installed; what it would write for these arrays is numpy.savetxt(..., '%.18g') per record, which
tests/test_result_text_restatement.py holds the restatement to).
Stored: the inputs, per writer the element names, the text flag and every captured column, get_color_from_label for every
label of the four datasets, and error2ply's colours on the 2000 vertices of result_text_cases.error_case().
    python tools/gen_result_text_golden.py"""
import colorsys
import os
import random
import re
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import result_text_cases as C  # noqa: E402
from gen_edgeloss_golden import REF  # noqa: E402

FUNCTIONS = ('partition2ply', 'geof2ply', 'prediction2ply', 'error2ply', 'spg2ply', 'scalar2ply', 'get_color_from_label', 'write_ply_obj',
             'write_ply_labels', 'write_ply')
WRITTEN = []                   # (file name, text flag, [(element name, structured array), ...]), call by call


class PlyElement:
    def __init__(self, data, name):
        self.data, self.name = np.array(data), name

    @staticmethod
    def describe(data, name):
        return PlyElement(data, name)


class PlyData:
    def __init__(self, elements, text=False):
        self.elements, self.text = list(elements), text

    def write(self, filename):
        WRITTEN.append((filename, self.text, [(e.name, e.data) for e in self.elements]))


def load():
    with open(os.path.join(REF, 'partition', 'provider.py')) as f:
        lines = f.read().split('\n')
    mod = types.ModuleType('ref_provider')
    mod.__dict__.update(np=np, random=random, colorsys=colorsys, PlyData=PlyData, PlyElement=PlyElement)
    for name in FUNCTIONS:
        first = next(i for i, line in enumerate(lines) if line.startswith(f'def {name}('))
        last = next(i for i in range(first + 1, len(lines)) if re.match(r'(def|import|from|class)\b', lines[i]))
        exec(compile('\n' * first + '\n'.join(lines[first:last]), os.path.join(REF, 'partition', 'provider.py'), 'exec'), mod.__dict__)
    return mod


def main():
    if not os.path.isdir(REF):
        sys.exit(f'reference checkout not found at {REF}')
    mod = load()
    c = C.cloud_case()
    out = {f'in/{k}': v for k, v in c.items() if isinstance(v, np.ndarray)}
    for i, comp in enumerate(c['components']):
        out[f'in/components/{i}'] = comp
    calls = {
        'write_ply': lambda f: mod.write_ply(f, c['xyz'], c['rgb']),
        'write_ply_labels': lambda f: mod.write_ply_labels(f, c['xyz'], c['rgb'], c['labels']),
        'write_ply_obj': lambda f: mod.write_ply_obj(f, c['xyz'], c['rgb'], c['labels'], c['object_indices']),
        'partition2ply': lambda f: mod.partition2ply(f, c['xyz'], c['components']),
        'geof2ply': lambda f: mod.geof2ply(f, c['xyz'], c['geof']),
        'prediction2ply': lambda f: mod.prediction2ply(f, c['xyz'], c['labels'], C.N_LABEL, C.DATASET),
        'prediction2ply_hist': lambda f: mod.prediction2ply(f, c['xyz'], c['histograms'], C.N_LABEL, C.DATASET),
        'error2ply': lambda f: mod.error2ply(f, c['xyz'], c['rgb'], c['labels'], c['histograms']),
        'spg2ply': lambda f: mod.spg2ply(f, {k: c[k] for k in ('sp_centroids', 'source', 'target')}),
        'scalar2ply': lambda f: mod.scalar2ply(f, c['xyz'], c['scalar']),
    }
    for name, call in calls.items():
        WRITTEN.clear()
        random.seed(C.SEED)
        with np.errstate(invalid='ignore'):                     # (geof2ply's colours above 255)
            call(name + '.ply')
        (filename, text, elements), = WRITTEN
        assert filename == name + '.ply'
        out[f'{name}/text'] = np.bool_(text)
        out[f'{name}/elements'] = np.array([e for e, _ in elements])
        for element, data in elements:
            out[f'{name}/{element}/properties'] = np.array(data.dtype.names)
            for prop in data.dtype.names:
                out[f'{name}/{element}/{prop}'] = np.ascontiguousarray(data[prop])
    for dataset, n in C.DATASETS.items():
        out[f'colour/{dataset}'] = np.array([mod.get_color_from_label(i, dataset) for i in range(n)], dtype=np.uint8)
    e = C.error_case()
    WRITTEN.clear()
    mod.error2ply('e.ply', np.zeros((len(e['rgb']), 3), np.float32), e['rgb'], e['labels'], e['prediction'])
    data = WRITTEN[0][2][0][1]
    out['error/colour'] = np.stack([data['red'], data['green'], data['blue']], axis=1)
    path = os.path.join(ROOT, 'tests', 'golden', 'result_text.npz')
    np.savez_compressed(path, **out)
    for k in sorted(out):
        print(f'{k:48s} {str(out[k].dtype):8s} {out[k].shape}')
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
