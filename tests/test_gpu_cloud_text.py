"""GPU: the raw cloud readers (csrc/spg_text.hip through ops.parse_cloud_text / ops.CloudTextReader and the three functions of
partition/provider.py).  Neither the reference nor pandas is read here: the judges are the plain Python restatement
(tests/cloud_text_restatement.py, itself held to pandas and to the reference's results on the CPU) and the reference's results
stored in tests/golden/cloud_text.npz.  Everything is bit for bit.

* every accepted case (tests/cloud_text_cases.py; the tile-edge cases placed from the library's own layout) equals the
  restatement, twice with the same bits;
* CloudTextReader yields the same rows for every block size that cuts a line;
* every refusal raises ValueError with the expected code, line and offset, and a good buffer parses after it (malformed input
  handled by design: the kernels bound every read by the buffer and the line cap);
* read_semantic3d_format, read_s3dis_format and interpolate_labels_batch equal the golden, chunk by chunk and in their results;
* a 200 000-line file parsed whole equals the same file read in 7 blocks."""
import glob
import os

import numpy as np
import pytest
import torch

import cloud_text_cases as C
import cloud_text_restatement as R
from conftest import GOLDEN
from oracle import spg_partition_oracle as PO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops(hip):
    from superpoint_graph_amd import ops
    return ops


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'cloud_text.npz'))


@pytest.fixture(scope='module')
def parse_cases(ops):
    return dict(C.parse_cases(ops.text_layout()))


@pytest.fixture(scope='module')
def refusal_cases(ops):
    return dict(C.refusal_cases(ops.text_layout()))


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = np.asarray(b)
    if b.dtype.kind == 'f':
        b = b + b.dtype.type(0)                     # (the device writes +0.0 itself: only the judge is normalised)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def spec_of(case):
    return {k: case[k] for k in ('n_cols', 'xyz_cols', 'rgb_cols', 'label_col')}


def device_bytes(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device='cuda')


def write(folder, name, data):
    path = os.path.join(str(folder), name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'wb') as f:
        f.write(data)
    return path


def test_layout_is_what_the_cases_assume(ops):
    layout = ops.text_layout()
    assert layout['index_tile'] % 16 == 0 and 1024 <= layout['index_tile'] <= 65536 and layout['max_line'] == R.MAX_LINE


@pytest.mark.parametrize('name', [n for n, _ in C.parse_cases()])
def test_parse_equals_restatement(ops, parse_cases, name):
    c = parse_cases[name]
    ref = R.parse(c['data'], **spec_of(c))
    text = device_bytes(c['data'])
    for run in range(2):                            # (the second run: the same bits again)
        out = ops.parse_cloud_text(text, **spec_of(c))
        assert out[3:] == ref[3:], (run, out[3:], ref[3:])
        for a, b, what in zip(out[:3], ref[:3], ('xyz', 'rgb', 'label')):
            assert same_bits(a, b), (run, what)
    # a block that is not the last: the unterminated tail is left to the caller
    open_ref = R.parse(c['data'], final_block=False, **spec_of(c))
    out = ops.parse_cloud_text(text, final_block=False, **spec_of(c))
    assert out[3:] == open_ref[3:] and all(same_bits(a, b) for a, b in zip(out[:3], open_ref[:3]))
    # (a view that starts off the 16-byte grid)
    shifted = torch.cat((torch.zeros(3, dtype=torch.uint8, device='cuda'), text))[3:]
    out = ops.parse_cloud_text(shifted, **spec_of(c))
    assert out[3:] == ref[3:] and all(same_bits(a, b) for a, b in zip(out[:3], ref[:3]))


@pytest.mark.parametrize('name', [n for n, _ in C.carry_cases()])
def test_reader_rows_do_not_depend_on_the_block_size(ops, tmp_path, name):
    c = dict(C.carry_cases())[name]
    path = write(tmp_path, 'cloud.txt', c['data'])
    ref = list(R.batches(c['data'], c['rows'], **spec_of(c)))
    assert [len(b[0]) for b in ref] == [3, 3, 1]
    for block in c['blocks']:
        got = list(ops.CloudTextReader(path, rows=c['rows'], block_bytes=block, **spec_of(c)))
        assert len(got) == len(ref), block
        for g, r in zip(got, ref):
            assert all(same_bits(a, b) for a, b in zip(g, r)), block
    skipped = list(ops.CloudTextReader(path, rows=4, block_bytes=50, skip_lines=2, **spec_of(c)))
    ref = list(R.batches(c['data'], 4, 2, **spec_of(c)))
    assert [len(b[0]) for b in skipped] == [4, 1] and all(same_bits(a, b) for g, r in zip(skipped, ref) for a, b in zip(g, r))


@pytest.mark.parametrize('name', [n for n, _ in C.refusal_cases()])
def test_refusals_name_the_line_and_leave_the_device_usable(ops, refusal_cases, parse_cases, tmp_path, name):
    c = refusal_cases[name]
    with pytest.raises(ValueError) as e:
        ops.parse_cloud_text(device_bytes(c['data']), **spec_of(c))
    assert isinstance(e.value, ops.CloudTextError)
    assert (e.value.code, e.value.line, e.value.offset, e.value.refused) == c['error'] + (1,), str(e.value)
    assert f'line {c["error"][1]}' in str(e.value) and ops.TEXT_ERRORS[c['error'][0]] in str(e.value)
    # through the reader, in blocks that cut the refused line: the line and the offset are the file's
    path = write(tmp_path, 'bad.txt', c['data'])
    with pytest.raises(ops.CloudTextError) as e:
        list(ops.CloudTextReader(path, rows=2, block_bytes=c['error'][2] + 1, **spec_of(c)))
    assert (e.value.code, e.value.line, e.value.offset) == c['error'], str(e.value)
    good = parse_cases['lines_65']
    out = ops.parse_cloud_text(device_bytes(good['data']), **spec_of(good))
    assert same_bits(out[0], R.parse(good['data'], **spec_of(good))[0])


def test_several_refused_lines_report_the_first(ops, refusal_cases):
    data = b''.join(refusal_cases[n]['data'] for n in ('colour_256', 'nan', 'fields_6'))
    with pytest.raises(ops.CloudTextError) as e:
        ops.parse_cloud_text(device_bytes(data), **C.SEMA)
    with pytest.raises(R.Refused) as r:
        R.parse(data, **C.SEMA)
    assert (e.value.code, e.value.line, e.value.offset, e.value.refused) == (r.value.code, r.value.line, r.value.offset, 3)


def test_read_semantic3d_format_equals_the_golden(ops, golden, tmp_path, monkeypatch):
    from superpoint_graph_amd.partition import provider
    chunks = []
    real_prune = ops.prune

    def prune(xyz, voxel_size, rgb=None, labels=None, *args, **kw):
        chunks.append((xyz, rgb, labels))
        return real_prune(xyz, voxel_size, rgb, labels, *args, **kw)
    monkeypatch.setattr(ops, 'prune', prune)
    for name, c in C.semantic3d_cases():
        chunks.clear()
        data = write(tmp_path, f'{name}.txt', c['data'])
        labels = write(tmp_path, f'{name}.labels', c['labels']) if c['n_class'] else ''
        out = provider.read_semantic3d_format(data, c['n_class'], labels, c['voxel_width'], c['ver_batch'])
        ref = [k for k in range(int(golden[f'sema3d/{name}/n_chunks'])) if len(golden[f'sema3d/{name}/chunk{k}/xyz'])]
        assert len(chunks) == len(ref), name
        for (xyz, rgb, lab), k in zip(chunks, ref):
            assert same_bits(xyz, golden[f'sema3d/{name}/chunk{k}/xyz']) and same_bits(rgb, golden[f'sema3d/{name}/chunk{k}/rgb']), (name, k)
            if c['n_class']:
                assert same_bits(lab, golden[f'sema3d/{name}/chunk{k}/labels'][:len(xyz)]), (name, k)
        # the results: the golden's chunks through the numpy restatement of prune, stacked as provider.py:276-282 stacks them
        xyz, rgb = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8)
        hist = np.zeros((0, c['n_class'] + 1), np.uint32)
        for k in ref:
            lab = golden[f'sema3d/{name}/chunk{k}/labels'] if c['n_class'] else None
            x = golden[f'sema3d/{name}/chunk{k}/xyz']
            xs, cs, ls, _ = PO.prune(x, c['voxel_width'], golden[f'sema3d/{name}/chunk{k}/rgb'], None if lab is None else lab[:len(x)],
                                     None, c['n_class'], 0)
            xyz, rgb, hist = np.vstack((xyz, xs)), np.vstack((rgb, cs)), np.vstack((hist, ls))
        assert len(out) == (3 if c['n_class'] else 2)
        assert all(isinstance(a, np.ndarray) for a in out)
        assert same_bits(out[0], xyz) and same_bits(out[1], rgb), name
        if c['n_class']:
            assert same_bits(out[2], hist), name
        dev = provider.read_semantic3d_format(data, c['n_class'], labels, c['voxel_width'], c['ver_batch'], device=True)
        assert all(t.is_cuda for t in dev) and same_bits(dev[0], xyz)
    # first_line='data': every line, line k with label k
    c = dict(C.semantic3d_cases())['labelled_not_dividing']
    data, labels = write(tmp_path, 'every.txt', c['data']), write(tmp_path, 'every.labels', c['labels'])
    out = provider.read_semantic3d_format(data, c['n_class'], labels, c['voxel_width'], c['ver_batch'], first_line='data')
    ref = R.read_semantic3d_format(c['data'], c['labels'], c['n_class'], c['voxel_width'], c['ver_batch'], first_line='data')
    assert all(same_bits(a, b) for a, b in zip(out, ref)) and int(out[2].sum()) == 200
    with pytest.raises(NotImplementedError, match='CloudTextReader'):
        provider.read_semantic3d_format(data, c['n_class'], labels, 0, c['ver_batch'])


def test_interpolate_labels_batch_equals_the_golden(ops, golden, tmp_path):
    from superpoint_graph_amd.partition import provider
    for name, c in C.interpolate_cases():
        data = write(tmp_path, f'{name}.txt', c['data'])
        out = provider.interpolate_labels_batch(data, c['xyz'], c['labels'], c['ver_batch'])
        assert isinstance(out, np.ndarray) and same_bits(out, golden[f'interp/{name}/out']), name
        dev = provider.interpolate_labels_batch(data, c['xyz'], c['labels'], c['ver_batch'], device=True)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), golden[f'interp/{name}/out'])
    with pytest.raises(NotImplementedError):
        provider.interpolate_labels_batch(data, c['xyz'], c['labels'], 0)


def test_read_s3dis_format_equals_the_golden(ops, golden, tmp_path, monkeypatch):
    from superpoint_graph_amd.partition import provider
    real_glob = glob.glob
    monkeypatch.setattr(provider.glob, 'glob', lambda *a, **k: sorted(real_glob(*a, **k)))      # (as the generator fixes it)
    for name, c in C.s3dis_cases():
        room = write(tmp_path, f'{name}/{name}.txt', c['room'])
        for fname, data in c['objects']:
            write(tmp_path, f'{name}/Annotations/{fname}', data)
        out = provider.read_s3dis_format(room)
        assert len(out) == 4 and all(isinstance(a, np.ndarray) for a in out)
        for key, a in zip(('xyz', 'rgb', 'room_labels', 'room_object_indices'), out):
            assert same_bits(a, golden[f's3dis/{name}/{key}']), (name, key)
        xyz, rgb = provider.read_s3dis_format(room, label_out=False)
        assert same_bits(xyz, golden[f's3dis/{name}/xyz']) and same_bits(rgb, golden[f's3dis/{name}/rgb'])
        dev = provider.read_s3dis_format(room, device=True)
        assert all(t.is_cuda for t in dev) and np.array_equal(dev[3].cpu().numpy(), golden[f's3dis/{name}/room_object_indices'])
    assert provider.object_name_to_label('bookcase') == 10 and provider.object_name_to_label('stairs') == 0


def test_200k_lines_whole_equals_seven_blocks(ops, tmp_path):
    data = C.sema_text(77, 200_000)
    path = write(tmp_path, 'big.txt', data)
    whole = ops.parse_cloud_text(device_bytes(data), **C.SEMA)
    assert whole[3] == 200_000 and whole[4] == len(data)
    block = (len(data) + 6) // 7
    got = list(ops.CloudTextReader(path, rows=1 << 30, block_bytes=block, **C.SEMA))
    assert len(got) == 1 and -(-len(data) // block) == 7
    assert torch.equal(got[0][0].view(torch.int32), whole[0].view(torch.int32)) and torch.equal(got[0][1], whole[1])
    rows = np.arange(0, 200_000, 997)
    lines = data.split(b'\n')
    ref = R.parse(b'\n'.join(lines[r] for r in rows) + b'\n', **C.SEMA)
    assert same_bits(whole[0][torch.from_numpy(rows).cuda()], ref[0]) and same_bits(whole[1][torch.from_numpy(rows).cuda()], ref[1])
