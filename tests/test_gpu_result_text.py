"""GPU: the result writers (csrc/spg_format.hip through ops.text.format_table / ops.text.error_colours and the writers of
partition/provider.py).  Neither the reference nor plyfile is read here: the judges are the plain Python restatement
(tests/result_text_restatement.py, itself held to numpy.savetxt on the CPU) and the arrays the reference's own functions handed
to plyfile, stored in tests/golden/result_text.npz.  Every comparison is of bytes or integers.

* format_table equals the restatement byte for byte on every case of tests/result_text_cases.py, row_start included;
* a capacity one byte short raises and leaves the buffer untouched; bad dtype, device or column count raises before any launch;
* error_colours equals the golden and the restatement;
* every provider writer gives the restated header and the restatement of the golden's captured columns;
* write_label_file equals numpy.savetxt; write_semantic3d_labels equals the two-step form for every ver_batch."""
import io
import os
import random

import numpy as np
import pytest
import torch

import result_text_cases as C
import result_text_restatement as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def text(hip):
    from superpoint_graph_amd import ops
    return ops.text


@pytest.fixture(scope='module')
def provider(hip):
    from superpoint_graph_amd.partition import provider
    return provider


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'result_text.npz'))


@pytest.fixture(scope='module')
def tables():
    return C.table_cases()


def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a.size else torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device='cuda')


def device_columns(specs):
    """the same views as result_text_cases.resolve, over device copies"""
    out = []
    for spec in specs:
        t = on_device(spec[1])
        out.append(t if spec[0] in ('vec', 'mat') else t[:, spec[2]] if spec[0] == 'col' else t[::spec[2]])
    return out


def read(path):
    with open(path, 'rb') as f:
        return f.read()


def golden_elements(golden, writer):
    """[(element, [(property, captured column), ...]), ...] of one of the reference's writers"""
    return [(str(e), [(str(p), golden[f'{writer}/{e}/{p}']) for p in golden[f'{writer}/{e}/properties']]) for e in golden[f'{writer}/elements']]


def cloud(golden):
    c = {k[3:]: golden[k] for k in golden.files if k.startswith('in/') and not k.startswith('in/components/')}
    c['components'] = [golden[f'in/components/{i}'] for i in range(7)]
    return c


def test_format_table_equals_restatement(text, tables):
    assert len(tables) == 5 + 4 * len(C.ROW_COUNTS)
    for name, specs in tables:
        columns = C.columns_of(specs)
        got, row_start = text.format_table(device_columns(specs))
        want = R.table_bytes(columns)
        assert got.dtype == torch.uint8 and row_start.dtype == torch.int64 and got.is_cuda and row_start.is_cuda, name
        assert row_start.cpu().numpy().tolist() == R.row_starts(columns).tolist(), name
        assert got.cpu().numpy().tobytes() == want, name


def test_format_table_into_a_buffer(text):
    specs = dict(C.table_cases())['xyzrgbl_257']
    columns = device_columns(specs)
    want = R.table_bytes(C.columns_of(specs))
    assert text.format_table_capacity(columns) >= len(want)
    out = torch.full((len(want) + 24,), 0xA5, dtype=torch.uint8, device='cuda')
    got, row_start = text.format_table(columns, out=out)
    assert got.data_ptr() == out.data_ptr() and got.cpu().numpy().tobytes() == want and int(row_start[-1]) == len(want)
    assert out[len(want):].cpu().tolist() == [0xA5] * 24                           # nothing behind the text
    # one byte short: refused, nothing written
    short = torch.full((len(want) + 7,), 0x5A, dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match='smaller than the table'):
        text.format_table(columns, out=short[:len(want) - 1])
    torch.cuda.synchronize()
    assert short.cpu().tolist() == [0x5A] * (len(want) + 7)
    got, _ = text.format_table(columns, out=short[:len(want)])                     # exactly enough
    assert got.cpu().numpy().tobytes() == want and short[len(want):].cpu().tolist() == [0x5A] * 7


def test_format_table_refuses_bad_arguments(text):
    good = torch.zeros(5, dtype=torch.float32, device='cuda')
    with pytest.raises(TypeError):
        text.format_table([good.double()])
    with pytest.raises(TypeError):
        text.format_table([good, good.to(torch.int16)])
    with pytest.raises(RuntimeError):
        text.format_table([good.cpu()])
    with pytest.raises(RuntimeError):
        text.format_table([np.zeros(5, np.float32)])
    with pytest.raises(ValueError):
        text.format_table([good] * 17)
    with pytest.raises(ValueError):
        text.format_table([torch.zeros(5, 9, device='cuda'), torch.zeros(5, 8, device='cuda')])        # 17 once expanded
    with pytest.raises(ValueError):
        text.format_table([])
    with pytest.raises(ValueError):
        text.format_table([good, good[:4]])
    with pytest.raises(ValueError):
        text.format_table([torch.zeros(5, 2, 2, device='cuda')])
    with pytest.raises(ValueError):
        text.format_table([torch.zeros(5, 4, device='cuda')[:, :2]])                   # a matrix must be contiguous
    with pytest.raises(TypeError):
        text.format_table([good], out=torch.zeros(64, dtype=torch.int8, device='cuda'))
    with pytest.raises(RuntimeError):
        text.format_table([good], out=torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(ValueError):
        text.format_table([good], out=torch.zeros(64, dtype=torch.uint8, device='cuda')[1:])           # not 8-byte aligned
    got, _ = text.format_table([good])                                                 # and the library still works
    assert got.cpu().numpy().tobytes() == b'0\n' * 5


def test_error_colours(text, golden):
    e = C.error_case()
    got = text.error_colours(on_device(e['rgb']), on_device(e['labels']), on_device(e['prediction']))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), golden['error/colour'])
    assert np.array_equal(got.cpu().numpy(), R.error_colours(e['rgb'], e['labels'], e['prediction']))
    every = np.array([[r, g, b] for r in range(0, 256, 5) for g in range(0, 256, 3) for b in range(0, 256, 17)], dtype=np.uint8)
    for right in (0, 1):
        labels = np.ones(len(every), np.int64)
        got = text.error_colours(on_device(every), on_device(labels), on_device(labels + 1 - right))
        assert np.array_equal(got.cpu().numpy(), R.error_colours(every, labels, labels + 1 - right))
    assert text.error_colours(torch.empty(0, 3, dtype=torch.uint8, device='cuda'), torch.empty(0, dtype=torch.int64, device='cuda'),
                              torch.empty(0, dtype=torch.int64, device='cuda')).shape == (0, 3)
    with pytest.raises(TypeError):
        text.error_colours(on_device(every).float(), on_device(labels), on_device(labels))
    with pytest.raises(RuntimeError):
        text.error_colours(torch.from_numpy(every), on_device(labels), on_device(labels))


def test_provider_writers(provider, golden, tmp_path):
    P, c = provider, cloud(golden)
    spg = {k: c[k] for k in ('sp_centroids', 'source', 'target')}
    calls = {
        'write_ply': lambda f: P.write_ply(f, c['xyz'], c['rgb']),
        'write_ply_labels': lambda f: P.write_ply_labels(f, c['xyz'], c['rgb'], c['labels']),
        'write_ply_obj': lambda f: P.write_ply_obj(f, c['xyz'], c['rgb'], c['labels'], c['object_indices']),
        'partition2ply': lambda f: P.partition2ply(f, c['xyz'], c['components']),
        'geof2ply': lambda f: P.geof2ply(f, c['xyz'], c['geof']),
        'prediction2ply': lambda f: P.prediction2ply(f, c['xyz'], c['labels'], C.N_LABEL, C.DATASET),
        'prediction2ply_hist': lambda f: P.prediction2ply(f, c['xyz'], c['histograms'], C.N_LABEL, C.DATASET),
        'error2ply': lambda f: P.error2ply(f, c['xyz'], c['rgb'], c['labels'], c['histograms']),
        'spg2ply': lambda f: P.spg2ply(f, spg),
        'scalar2ply': lambda f: P.scalar2ply(f, c['xyz'], c['scalar']),
    }
    for name, call in calls.items():
        path = str(tmp_path / (name + '.ply'))
        random.seed(C.SEED)
        call(path)
        elements = golden_elements(golden, name)
        got, want = read(path), R.ply_bytes(elements)
        header = R.ply_header([(e, len(props[0][1]), [(p, a.dtype.str[1:]) for p, a in props]) for e, props in elements])
        assert got[:len(header)] == header, name
        assert got == want, name
    assert [e for e, _ in golden_elements(golden, 'spg2ply')] == ['vertex', 'edge']
    assert c['labels'][17] > C.N_LABEL                                                 # the out-of-range label went through prediction2ply


def test_provider_writers_take_device_tensors(provider, golden, tmp_path):
    P, c = provider, cloud(golden)
    d = {k: on_device(v) for k, v in c.items() if isinstance(v, np.ndarray) and v.dtype != np.uint32}
    path = str(tmp_path / 'a.ply')
    P.write_ply_labels(path, d['xyz'], d['rgb'], d['labels'])
    assert read(path) == R.ply_bytes(golden_elements(golden, 'write_ply_labels'))
    P.error2ply(path, d['xyz'], d['rgb'], d['labels'], d['histograms'])
    assert read(path) == R.ply_bytes(golden_elements(golden, 'error2ply'))
    P.geof2ply(path, d['xyz'], d['geof'])
    assert read(path) == R.ply_bytes(golden_elements(golden, 'geof2ply'))
    P.prediction2ply(path, d['xyz'], d['histograms'], C.N_LABEL, C.DATASET)
    assert read(path) == R.ply_bytes(golden_elements(golden, 'prediction2ply_hist'))


def test_partition2ply_colours_and_membership(provider, golden, tmp_path):
    P, c = provider, cloud(golden)
    want = R.ply_bytes(golden_elements(golden, 'partition2ply'))
    rgb = np.stack([golden[f'partition2ply/vertex/{k}'] for k in ('red', 'green', 'blue')], axis=1)
    colors = np.stack([rgb[comp[0]] for comp in c['components']])
    random.seed(C.SEED)
    assert colors.tolist() == [[random.randint(0, 255) for _ in range(3)] for _ in range(7)]
    in_component = np.full(C.N_VER, 7, dtype=np.int64)
    for i, comp in enumerate(c['components']):
        in_component[comp] = i
    assert (in_component == 7).sum() == 30 and not rgb[in_component == 7].any()        # vertices in no component stay black
    path = str(tmp_path / 'p.ply')
    P.partition2ply(path, c['xyz'], c['components'], colors=colors)
    assert read(path) == want
    P.partition2ply(path, c['xyz'], c['components'], colors=on_device(colors), in_component=on_device(in_component))
    assert read(path) == want
    with pytest.raises(ValueError):
        P.partition2ply(path, c['xyz'], c['components'], colors=colors[:6])


def test_writer_edges(provider, golden, tmp_path):
    P, c = provider, cloud(golden)
    path = str(tmp_path / 'e.ply')
    P.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))          # an empty cloud: the header alone
    assert read(path) == R.ply_header([('vertex', 0, [(p, 'f4') for p in 'xyz'] + [(p, 'u1') for p in ('red', 'green', 'blue')])])
    P.spg2ply(path, dict(sp_centroids=np.zeros((0, 3), np.float32), source=np.zeros((0, 1), np.int64), target=np.zeros((0, 1), np.int64)))
    assert read(path) == R.ply_header([('vertex', 0, [(p, 'f4') for p in 'xyz']), ('edge', 0, [('vertex1', 'i4'), ('vertex2', 'i4')])])
    with pytest.raises(ValueError, match='Unknown dataset'):
        P.prediction2ply(path, c['xyz'], c['labels'], C.N_LABEL, 'nuscenes')
    with pytest.raises(ValueError, match='Type not recognized'):
        P.prediction2ply(path, c['xyz'], c['labels'], 9, 'sema3d')                     # label 9 has no colour, as in the reference
    for dataset, n in C.DATASETS.items():
        assert [P.get_color_from_label(i, dataset) for i in range(n)] == golden[f'colour/{dataset}'].tolist()
        with pytest.raises(ValueError, match='Type not recognized'):
            P.get_color_from_label(n, dataset)
    with pytest.raises(ValueError, match='Unknown dataset'):
        P.get_color_from_label(0, 'nuscenes')
    bad = c['geof'].copy()
    bad[5, 1] = np.nan
    with pytest.raises(ValueError):
        P.geof2ply(path, c['xyz'], bad)
    bad[5, 1] = 2.0 ** 31 / 255 * 1.01
    with pytest.raises(ValueError):
        P.geof2ply(path, c['xyz'], bad)


def test_write_ply_in_blocks(provider, golden, tmp_path):
    """the private helper with a block of BLOCK_ROWS rows: 300 vertices in three blocks, and two elements"""
    P = provider
    assert C.N_VER > 2 * C.BLOCK_ROWS and 257 > 2 * C.BLOCK_ROWS
    codes = {'float32': 'f4', 'uint8': 'u1', 'uint32': 'u4', 'int32': 'i4'}
    for writer in ('write_ply_obj', 'spg2ply'):
        elements = golden_elements(golden, writer)
        device = [(e, [(p, codes[a.dtype.name], on_device(a.astype(np.int64) if a.dtype == np.uint32 else a)) for p, a in props]) for e, props in elements]
        path = str(tmp_path / (writer + '.ply'))
        P._write_ply(path, device, block_rows=C.BLOCK_ROWS)
        assert read(path) == R.ply_bytes(elements), writer
    specs = dict(C.table_cases())['strided7_257']
    path = str(tmp_path / 't.txt')
    with open(path, 'wb') as f:
        P._RowWriter(f, block_rows=C.BLOCK_ROWS).write(device_columns(specs))
    assert read(path) == R.table_bytes(C.columns_of(specs))


def test_write_label_file(provider, tmp_path):
    P = provider
    path = str(tmp_path / 'l.labels')
    rng = np.random.default_rng(3)
    cases = [np.arange(256, dtype=np.uint8), rng.integers(0, 9, 257).astype(np.uint8), rng.integers(-5, 10 ** 12, 65).astype(np.int64),
             rng.integers(0, 9, 64).astype(np.int32), rng.integers(0, 300, 63).astype(np.uint16), np.zeros(0, np.uint8)]
    for labels in cases:
        for offset in (1, 0):
            stream = io.BytesIO()
            np.savetxt(stream, labels + offset, delimiter=' ', fmt='%d')
            P.write_label_file(path, labels, offset, block_rows=C.BLOCK_ROWS)
            assert read(path) == stream.getvalue(), (labels.dtype, len(labels), offset)
            if labels.dtype != np.uint16:
                P.write_label_file(path, on_device(labels), offset)
                assert read(path) == stream.getvalue(), (labels.dtype, len(labels), offset)
    with pytest.raises(ValueError):
        P.write_label_file(path, np.zeros(4, np.float32))


@pytest.fixture(scope='module')
def label_cloud(provider, tmp_path_factory):
    """the 1000-line cloud on disk, the labels interpolate_labels_batch gives for it (vector and histograms) and their
    numpy.savetxt text: computed once"""
    c = C.label_cloud_case()
    folder = tmp_path_factory.mktemp('sema3d_labels')
    data = str(folder / 'cloud.txt')
    with open(data, 'wb') as f:
        f.write(c['data'])
    want = {}
    for key in ('labels', 'histograms'):
        ups = provider.interpolate_labels_batch(data, c['xyz'], c[key], 333)
        stream = io.BytesIO()
        np.savetxt(stream, ups + 1, delimiter=' ', fmt='%d')
        two_step = str(folder / f'two_step_{key}.labels')
        provider.write_label_file(two_step, ups)
        assert read(two_step) == stream.getvalue() and len(ups) == 1000
        want[key] = stream.getvalue()
    return dict(c, path=data, folder=folder, want=want)


@pytest.mark.parametrize('ver_batch', [1, 64, 333, 5000])
def test_write_semantic3d_labels(provider, label_cloud, ver_batch):
    c = label_cloud
    out = str(c['folder'] / f'streamed_{ver_batch}.labels')
    assert provider.write_semantic3d_labels(c['path'], c['xyz'], c['labels'], out, ver_batch) == 1000
    assert read(out) == c['want']['labels']
    if ver_batch != 1:
        assert provider.write_semantic3d_labels(c['path'], c['xyz'], c['histograms'], out, ver_batch) == 1000
        assert read(out) == c['want']['histograms']


def test_write_semantic3d_labels_refusals(provider, label_cloud):
    c = label_cloud
    out = str(c['folder'] / 'refused.labels')
    with pytest.raises(NotImplementedError):
        provider.write_semantic3d_labels(c['path'], c['xyz'], c['labels'], out, 0)
    with pytest.raises(ValueError):
        provider.write_semantic3d_labels(c['path'], c['xyz'], c['labels'][:-1], out, 100)
