"""CPU: the plain Python restatement of the raw cloud readers (tests/cloud_text_restatement.py) against the reference's own
results (tests/golden/cloud_text.npz, tools/gen_cloud_text_golden.py) and against pandas.read_csv where it is installed; the
cases (tests/cloud_text_cases.py) are what they claim to be.  Everything is compared bit for bit, after `+ 0.0` on floats (the
contract writes every zero as +0.0)."""
import io
import os

import numpy as np
import pytest

import cloud_text_cases as C
import cloud_text_restatement as R
from conftest import ROOT

PARSE = C.parse_cases()
REFUSALS = C.refusal_cases()


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'cloud_text.npz'))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == 'f':
        a, b = a + a.dtype.type(0), b + b.dtype.type(0)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def spec_of(case):
    return {k: case[k] for k in ('n_cols', 'xyz_cols', 'rgb_cols', 'label_col')}


def test_cases_cover_the_claimed_sizes_and_edges():
    by_name = dict(PARSE)
    counts = {name: R.parse(c['data'], **spec_of(c))[3] for name, c in PARSE}
    assert [counts[f'lines_{n}'] for n in (0, 1, 63, 64, 65, 255, 256, 257)] == [0, 1, 63, 64, 65, 255, 256, 257]
    assert max(counts.values()) <= 300
    assert counts['blank_lines'] == 9 and counts['only_blank'] == 0 and counts['crlf'] == 70
    assert not by_name['no_final_newline']['data'].endswith(b'\n') and by_name['crlf_no_final']['data'].count(b'\r\n') == 3
    for k in (1, 3):
        edge = k * C.DEFAULT_LAYOUT['index_tile']
        assert by_name[f'tile_{k}_newline_last_byte']['data'][edge - 1:edge] == b'\n'
        assert by_name[f'tile_{k}_newline_first_byte']['data'][edge:edge + 1] == b'\n'
        assert by_name[f'tile_{k}_token_across']['data'][edge - 4:edge + 5] == b'\n-12.3456'
    longest = max(len(c) for _, c in R.lines_of(by_name['max_line_exact']['data'])[0])
    assert longest == C.DEFAULT_LAYOUT['max_line'] == R.MAX_LINE
    for name, c in C.carry_cases():
        lines = R.lines_of(c['data'])[0]
        start, content = lines[2]
        assert set(range(start, start + len(content) + 2)) <= set(c['blocks']) and min(c['blocks']) == 1


def test_token_values_known_answers():
    xyz = R.parse(dict(PARSE)['tokens']['data'], **C.SEMA)[0]
    expect = np.array([[0, 0, 0], [.5, 5, 1.5], [.25, 123456789.012345, -1.23456789e-8], [-.5, 0, -5],
                       [999999999999999, 1e-15, 1.5], [.1, .7, -.3]], dtype=np.float64).astype(np.float32)
    assert same_bits(xyz, expect) and not np.signbit(xyz[0]).any()
    xyz = R.parse(dict(PARSE)['tokens_past_pandas']['data'], **C.SEMA)[0]
    expect = np.array([[-1e-22, 1.5, 1.2345678e-15], [1.23456789012345e-8, 12.75, -.5]], dtype=np.float64).astype(np.float32)
    assert same_bits(xyz, expect)
    rgb = R.parse(dict(PARSE)['colours']['data'], **C.SEMA)[1]
    assert rgb.tolist() == [[0, 255, 12], [255, 0, 7]]


@pytest.mark.parametrize('name', [n for n, c in PARSE if c.get('pandas', True)])
def test_restatement_equals_pandas(name):
    """(tokens_past_pandas is left out: pandas keeps the first 17 digits of a token, leading zeros included, and its value for
    `-0.0000000000000000000001` is -0.0; the contract's value is the correctly rounded one, float()'s)"""
    pd = pytest.importorskip('pandas')
    c = dict(PARSE)[name]
    xyz, rgb, label, n, _ = R.parse(c['data'], **spec_of(c))
    if n == 0:
        with pytest.raises(pd.errors.EmptyDataError):
            pd.read_csv(io.BytesIO(c['data']), sep=' ', header=None)
        return
    if c['label_col'] is not None:                  # provider.py:291
        values = pd.read_csv(io.BytesIO(c['data']), dtype='u1', header=None).values
        assert same_bits(values.squeeze(), label)
        return
    values = pd.read_csv(io.BytesIO(c['data']), sep=' ', header=None).values
    assert values.shape == (n, c['n_cols'])
    assert same_bits(np.ascontiguousarray(np.array(values[:, list(c['xyz_cols'])], dtype='float32')), xyz)      # :266 / :190
    assert same_bits(np.ascontiguousarray(np.array(values[:, list(c['rgb_cols'])], dtype='uint8')), rgb)        # :267 / :192


@pytest.mark.parametrize('name', [n for n, _ in REFUSALS])
def test_refusal_cases_are_outside_the_grammar(name):
    c = dict(REFUSALS)[name]
    with pytest.raises(R.Refused) as e:
        R.parse(c['data'], **spec_of(c))
    assert (e.value.code, e.value.line, e.value.offset) == c['error'] and e.value.refused == 1
    lines = R.lines_of(c['data'])[0]
    good = [R.refusal(s, content, R.roles_of(**spec_of(c))) for s, content in lines]
    assert [g is None for g in good] == [True, False, True]


def test_restatement_equals_the_reference_semantic3d(golden):
    for name, c in C.semantic3d_cases():
        chunks = R.semantic3d_chunks(c['data'], c['labels'], c['n_class'], c['ver_batch'])
        ref = [k for k in range(int(golden[f'sema3d/{name}/n_chunks'])) if len(golden[f'sema3d/{name}/chunk{k}/xyz'])]
        assert len(chunks) == len(ref), name
        for (xyz, rgb, labels), k in zip(chunks, ref):
            assert same_bits(xyz, golden[f'sema3d/{name}/chunk{k}/xyz']), (name, k)
            assert same_bits(rgb, golden[f'sema3d/{name}/chunk{k}/rgb']), (name, k)
            if c['n_class']:
                assert same_bits(labels, golden[f'sema3d/{name}/chunk{k}/labels']), (name, k)
        # the generator's prune hands the points back: the function's outputs are the chunks stacked (labels: empty histograms)
        stack = np.vstack([np.zeros((0, 3), np.float32)] + [x for x, _, _ in chunks])
        assert same_bits(stack, golden[f'sema3d/{name}/out_xyz']), name
        assert same_bits(np.vstack([np.zeros((0, 3), np.uint8)] + [x for _, x, _ in chunks]), golden[f'sema3d/{name}/out_rgb']), name
        out = R.read_semantic3d_format(c['data'], c['labels'], c['n_class'], c['voxel_width'], c['ver_batch'])
        assert len(out) == (3 if c['n_class'] else 2) and len(out[0]) <= len(stack)
        if c['n_class']:
            assert golden[f'sema3d/{name}/out_labels'].dtype == out[2].dtype == np.uint32
            assert out[2].shape == (len(out[0]), c['n_class'] + 1) and int(out[2].sum()) == len(stack)
    # 'data' keeps the first line: one point more than 'reference', paired with its own label
    c = dict(C.semantic3d_cases())['labelled_not_dividing']
    every = R.semantic3d_chunks(c['data'], c['labels'], c['n_class'], c['ver_batch'], first_line='data')
    assert sum(len(x) for x, _, _ in every) == 200 and same_bits(every[0][0][1:], R.semantic3d_chunks(
        c['data'], c['labels'], c['n_class'], c['ver_batch'])[0][0][:63])


def test_restatement_equals_the_reference_interpolation(golden):
    for name, c in C.interpolate_cases():
        out = R.interpolate_labels_batch(c['data'], c['xyz'], c['labels'], c['ver_batch'])
        assert same_bits(out, golden[f'interp/{name}/out']), name


def test_restatement_equals_the_reference_s3dis(golden):
    from superpoint_graph_amd.partition.provider import object_name_to_label
    for name, c in C.s3dis_cases():
        objects = [(object_name_to_label(f.split('_')[0]), data) for f, data in sorted(c['objects'])]
        out = R.read_s3dis_format(c['room'], objects)
        for key, a in zip(('xyz', 'rgb', 'room_labels', 'room_object_indices'), out):
            assert same_bits(a, golden[f's3dis/{name}/{key}']), (name, key)
        assert len(set(out[3].tolist())) == 4 and 0 in out[3]            # three objects and untouched points


def test_s3dis_cases_have_no_equidistant_candidates():
    import knn_restatement as KR
    for name, c in C.s3dis_cases():
        room = R.parse(c['room'], **C.S3DIS)[0]
        for _, data in c['objects']:
            d2 = np.sort(KR.d2_rows(R.parse(data, 6, (0, 1, 2))[0], room), axis=1)
            assert (d2[:, 0] < d2[:, 1]).all(), name
