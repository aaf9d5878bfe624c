"""CPU: the plain Python restatement of the result text (tests/result_text_restatement.py), which judges csrc/spg_format.hip and
the writers of partition/provider.py on the GPU, is itself held to numpy.savetxt -- '%.18g' record by record, as plyfile's text
writer calls it (plyfile is not installed: UNPINNED against it), and '%d' for labels -- byte for byte on every case of
tests/result_text_cases.py, and to what the reference's own functions computed (tests/golden/result_text.npz)."""
import ctypes
import io
import os

import numpy as np
import pytest

import result_text_cases as C
import result_text_restatement as R
from conftest import GOLDEN


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'result_text.npz'))


@pytest.fixture(scope='module')
def tables():
    return C.table_cases()


def test_ties_exist():
    ties = C.tie_f32()
    assert len(ties) >= 15
    assert '%.18g' % float(np.float32(12345677 * 2.0 ** -16)) == '188.380081176757812'
    assert '%.18g' % float(np.float32(16777215 * 2.0 ** -16)) == '255.999984741210938'
    assert R.field(np.float32(1e18)) == '999999984306749440' and R.field(np.nextafter(np.float32(1e18), np.float32(np.inf))).endswith('e+18')
    assert R.field(np.array([1], dtype=np.uint32).view(np.float32)[0]) == '1.40129846432481707e-45'


def test_float_fields_equal_savetxt():
    """'%.18g' through numpy.savetxt on the float32 column, record by record as plyfile does and as one call"""
    values = C.all_f32()
    want = R.table_bytes([values])
    stream = io.BytesIO()
    np.savetxt(stream, values, '%.18g')
    assert stream.getvalue() == want
    head = np.concatenate((C.special_f32(), C.tie_f32(), C.random_f32()[:2000]))
    stream = io.BytesIO()
    for v in head:
        np.savetxt(stream, [v], '%.18g', newline='\n')
    assert stream.getvalue() == R.table_bytes([head])


def test_float_fields_round_trip():
    """np.float32(float(field)) gives back every finite input bit for bit"""
    values = C.all_f32()
    finite = values[np.isfinite(values)]
    back = np.array([float(R.field(v)) for v in finite], dtype=np.float64).astype(np.float32)
    assert back.view(np.uint32).tolist() == finite.view(np.uint32).tolist()
    other = values[~np.isfinite(values)]
    assert sorted({R.field(v) for v in other}) == ['-inf', 'inf', 'nan']


def test_integer_fields_equal_savetxt():
    for name, values in C.int_cases().items():
        stream = io.BytesIO()
        np.savetxt(stream, values, delimiter=' ', fmt='%d')
        assert stream.getvalue() == R.table_bytes([values]), name


def test_tables_equal_savetxt_per_record(tables):
    """a record of mixed fields, as plyfile hands it to numpy.savetxt: a list of Python scalars, '%.18g' for every one (an integer
    field prints the same under '%.18g' as under '%d' up to 18 digits; the int64 columns of the cases go beyond, so the integer
    columns are held to '%d')"""
    for name, specs in tables:
        if name == 'f32_all':
            continue
        columns = C.columns_of(specs)
        stream = io.BytesIO()
        fmt = ['%d' if c.dtype.kind in 'iu' else '%.18g' for c in columns]
        for row in zip(*columns):
            np.savetxt(stream, [np.array([int(v) if isinstance(v, np.integer) else float(v) for v in row], dtype=object)], fmt, newline='\n')
        want = R.table_bytes(columns)
        assert stream.getvalue() == want, name
        starts = R.row_starts(columns)
        assert starts[-1] == len(want) and len(starts) == len(columns[0]) + 1
        assert all(want[a:b].endswith(b'\n') and b' \n' not in want[a:b] and b'\r' not in want[a:b] for a, b in zip(starts[:-1], starts[1:]))


def test_small_integers_print_alike_under_both_formats():
    """plyfile prints u1 / i4 / u4 properties with '%.18g' too: the same text as '%d' for every value of those types"""
    for values in (np.arange(256), np.array([-2 ** 31, 2 ** 31 - 1, 2 ** 32 - 1, 10 ** 9, -10 ** 9, 123456789])):
        assert all('%.18g' % int(v) == '%d' % int(v) for v in values)


def test_headers(golden):
    want = b'ply\nformat ascii 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\nelement edge 12\n' \
           b'property int vertex1\nproperty int vertex2\nend_header\n'
    assert R.ply_header([('vertex', 7, [('x', 'f4'), ('y', 'f4'), ('z', 'f4')]), ('edge', 12, [('vertex1', 'i4'), ('vertex2', 'i4')])]) == want
    assert list(golden['spg2ply/elements']) == ['vertex', 'edge'] and golden['spg2ply/edge/vertex1'].dtype == np.int32
    want = b'ply\nformat ascii 1.0\nelement vertex 300\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n' \
           b'property uchar green\nproperty uchar blue\nproperty uchar label\nproperty uint object_index\nend_header\n'
    props = [(str(p), golden[f'write_ply_obj/vertex/{p}'].dtype.str[1:]) for p in golden['write_ply_obj/vertex/properties']]
    assert R.ply_header([('vertex', 300, props)]) == want
    for key in golden.files:
        if key.endswith('/text'):
            assert bool(golden[key]), key                                       # every writer asked for text=True


def test_error_colours_equal_the_reference(golden):
    e = C.error_case()
    assert len(e['rgb']) == 2000
    assert np.array_equal(R.error_colours(e['rgb'], e['labels'], e['prediction']), golden['error/colour'])
    hist = np.argmax(golden['in/histograms'], axis=1)
    got = R.error_colours(golden['in/rgb'], golden['in/labels'], hist)
    want = np.stack([golden[f'error2ply/vertex/{c}'] for c in ('red', 'green', 'blue')], axis=1)
    assert np.array_equal(got, want)


def test_golden_inputs_are_the_cases(golden):
    c = C.cloud_case()
    for k, v in c.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(golden[f'in/{k}'], v, equal_nan=True) and golden[f'in/{k}'].dtype == v.dtype, k
    assert all(np.array_equal(golden[f'in/components/{i}'], comp) for i, comp in enumerate(c['components']))
    assert np.array_equal(golden['prediction2ply/vertex/red'][17:18], [0]) and c['labels'][17] > C.N_LABEL
    # geof2ply: wherever 255 * v lies in [0, 256) the colour is the truncation; above it, the low byte of the int32 truncation
    scaled = 255 * c['geof'][:, [0, 1, 3]]
    want = (scaled.astype(np.int32) & 255).astype(np.uint8)
    got = np.stack([golden[f'geof2ply/vertex/{k}'] for k in ('red', 'green', 'blue')], axis=1)
    assert (scaled >= 256).any() and np.array_equal(got, want)


def test_field_formatter_on_the_host(hip):
    """the library's own field formatter (the function the kernels run, compiled for the host too: spg_format_debug_field)
    against Python's % operator; no device is touched"""
    L = hip
    buf = ctypes.create_string_buffer(32)

    def fields(kind, values):
        out = []
        for i in range(len(values)):
            n = L.spg_format_debug_field(kind, values[i:i + 1].ctypes.data, buf)
            out.append(buf.raw[:n])
        return b'\n'.join(out) + b'\n'
    floats = np.concatenate((C.special_f32(), C.tie_f32(), C.random_f32()[:20000]))
    assert fields(4, floats) == R.table_bytes([floats])
    for kind, name in ((0, 'uint8'), (1, 'int32'), (2, 'uint32'), (3, 'int64')):
        values = C.int_cases()[name]
        assert fields(kind, values) == R.table_bytes([values]), name
