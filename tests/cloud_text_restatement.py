"""Plain Python restatement of the raw cloud readers (csrc/spg_text.hip, ops.parse_cloud_text, partition/provider.py): lines by
bytes.split, fields by split(' '), values by float() -> np.float32 -> + 0.0, the grammar by a regular expression, and the
chunking of read_semantic3d_format / read_s3dis_format / interpolate_labels_batch on top of the numpy restatements of prune
(oracle/spg_partition_oracle.py) and of the 1-nearest neighbour (tests/knn_restatement.py)."""
import re

import numpy as np

import knn_restatement as KR
from oracle import spg_partition_oracle as PO

FIELDS, EMPTY, BYTE, TOKEN, RANGE, LONG = 1, 2, 3, 4, 5, 6
MAX_LINE, MAX_DIGITS, MAX_FRACTION = 512, 15, 22
_NUMBER = re.compile(rb'[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)')
_ALLOWED = frozenset(b'0123456789.+-')


class Refused(Exception):
    def __init__(self, line, code, offset, refused=1):
        super().__init__(f'line {line} code {code} offset {offset} ({refused} refused)')
        self.line, self.code, self.offset, self.refused = line, code, offset, refused


def lines_of(data, final_block=True):
    """-> ([(start offset, the bytes in front of the terminator)] of the non-blank lines, consumed)."""
    out, pos = [], 0
    pieces = data.split(b'\n')
    tail = pieces.pop()                              # behind the last '\n' (empty when the data ends with one)
    for piece in pieces:
        content = piece[:-1] if piece.endswith(b'\r') else piece
        if content:
            out.append((pos, content))
        pos += len(piece) + 1
    if final_block:
        if tail:
            out.append((pos, tail))
        pos = len(data)
    return out, pos


def token_ok(tok):
    if not _NUMBER.fullmatch(tok):
        return False
    digits = tok.lstrip(b'+-')
    whole, _, frac = digits.partition(b'.')
    return len((whole + frac).lstrip(b'0')) <= MAX_DIGITS and len(frac) <= MAX_FRACTION


def roles_of(n_cols, xyz_cols, rgb_cols, label_col):
    roles = [-1] * n_cols
    for cols, first in ((xyz_cols, 0), (rgb_cols, 3)):
        if cols is not None:
            for k, c in enumerate(cols):
                roles[c] = first + k
    if label_col is not None:
        roles[label_col] = 6
    return roles


def refusal(start, content, roles):
    """None, or (code, offset) of the first refusal met walking the line from the left: a byte is judged where it stands, a field
    at its end, the length where byte MAX_LINE of the line is reached."""
    events = []                                      # (where it is noticed, code, the offset reported)
    if len(content) > MAX_LINE:
        events.append((start + MAX_LINE - 0.5, LONG, start + MAX_LINE))      # (noticed in front of whatever stands there)
    fields, o = content.split(b' '), start
    for k, tok in enumerate(fields):
        end = o + len(tok)
        bad = [j for j, c in enumerate(tok) if c not in _ALLOWED]
        if not tok:
            events.append((o, EMPTY, o))
        elif bad:
            events.append((o + bad[0], BYTE, o + bad[0]))
        elif k >= len(roles):
            events.append((end, FIELDS, o))
        elif not token_ok(tok):
            events.append((end, TOKEN, o))
        elif roles[k] >= 3:
            v = float(tok)
            if not (v == int(v) and 0 <= v <= 255):
                events.append((end, RANGE, o))
        o = end + 1
    if len(fields) < len(roles):
        events.append((start + len(content) + 0.5, FIELDS, start + len(content)))
    if not events:
        return None
    _, code, where = min(events)
    return code, where


def parse(data, n_cols, xyz_cols=(0, 1, 2), rgb_cols=None, label_col=None, final_block=True):
    """-> (xyz f32 [n, 3] | None, rgb u8 [n, 3] | None, label u8 [n] | None, n, consumed); raises Refused."""
    roles = roles_of(n_cols, xyz_cols, rgb_cols, label_col)
    lines, consumed = lines_of(data, final_block)
    refused = [(i, refusal(s, c, roles)) for i, (s, c) in enumerate(lines)]
    refused = [(i, r) for i, r in refused if r is not None]
    if refused:
        i, (code, where) = refused[0]
        raise Refused(i, code, where, len(refused))
    rows = [[float(t) for t in c.split(b' ')] for _, c in lines]
    table = np.array(rows, dtype=np.float64).reshape(len(rows), n_cols)

    def pick(cols, dtype):
        return None if cols is None else np.ascontiguousarray(table[:, list(cols)].astype(dtype) + dtype(0))
    label = None if label_col is None else table[:, label_col].astype(np.uint8)
    return pick(xyz_cols, np.float32), pick(rgb_cols, np.uint8), label, len(rows), consumed


def batches(data, rows, skip_lines=0, **kw):
    """what ops.CloudTextReader yields: the parsed rows behind the first skip_lines, `rows` at a time."""
    xyz, rgb, label, n, _ = parse(data, **kw)
    for a in range(skip_lines, n, rows):
        yield tuple(None if t is None else t[a:a + rows] for t in (xyz, rgb, label))


# ---- the three provider functions ----
def semantic3d_chunks(data, labels_data, n_class, ver_batch, first_line='reference'):
    """[(xyz, rgb, labels | None)]: what every call of prune receives (labels as long as the reference's label chunk)."""
    skip = 1 if n_class > 0 and first_line == 'reference' else 0
    points = batches(data, ver_batch, skip, n_cols=7, xyz_cols=(0, 1, 2), rgb_cols=(4, 5, 6))
    if n_class == 0:
        return [(x, c, None) for x, c, _ in points]
    label_lines = batches(labels_data, ver_batch, n_cols=1, xyz_cols=None, label_col=0)
    return [(x, c, lab) for (x, c, _), (_, _, lab) in zip(points, label_lines)]


def read_semantic3d_format(data, labels_data, n_class, voxel_width, ver_batch, first_line='reference'):
    xyz, rgb = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8)
    labels = np.zeros((0, n_class + 1), np.uint32)
    for x, c, lab in semantic3d_chunks(data, labels_data, n_class, ver_batch, first_line):
        xs, cs, ls, _ = PO.prune(x, voxel_width, c, None if lab is None else lab[:len(x)], None, n_class, 0)
        xyz, rgb = np.vstack((xyz, xs)), np.vstack((rgb, cs))
        if n_class > 0:
            labels = np.vstack((labels, ls))
    return (xyz, rgb, labels) if n_class > 0 else (xyz, rgb)


def nearest(ref_xyz, query_xyz):
    return KR.knn(ref_xyz, 1, query=query_xyz)[0].reshape(-1)


def read_s3dis_format(room_data, objects):
    """objects: [(label, the bytes of the annotation file)] in the order they are applied."""
    xyz, rgb, _, n, _ = parse(room_data, 6, (0, 1, 2), (3, 4, 5))
    room_labels, room_objects = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    for i, (label, data) in enumerate(objects, 1):
        obj_xyz = parse(data, 6, (0, 1, 2))[0]
        ind = nearest(xyz, obj_xyz)
        room_labels[ind], room_objects[ind] = label, i
    return xyz, rgb, room_labels, room_objects


def interpolate_labels_batch(data, xyz, labels, ver_batch, n_cols=7):
    labels = np.asarray(labels)
    if labels.ndim > 1 and labels.shape[1] > 1:
        labels = np.argmax(labels, axis=1)
    out = np.zeros((0,), dtype=np.uint8)
    for x, _, _ in batches(data, ver_batch, n_cols=n_cols, xyz_cols=(0, 1, 2)):
        out = np.hstack((out, labels[nearest(xyz, x)].flatten()))
    return out
