"""Named, seeded cases of the raw cloud readers: every case builds its file bytes itself (no text fixture is committed).
parse_cases(layout) -> the accepted buffers of ops.parse_cloud_text, refusal_cases() -> one buffer per refusal with the expected
(code, line, offset), carry_cases() -> files with the block sizes that cut one line at every byte, and the PARITY cases of the
three provider functions, which tools/gen_cloud_text_golden.py runs through the reference.  layout: ops.text_layout() on the
device, DEFAULT_LAYOUT elsewhere (the tile-edge cases are placed from it)."""
import random

import numpy as np

DEFAULT_LAYOUT = {'index_tile': 4096, 'max_line': 512}
FIELDS, EMPTY, BYTE, TOKEN, RANGE, LONG = 1, 2, 3, 4, 5, 6
SEMA = dict(n_cols=7, xyz_cols=(0, 1, 2), rgb_cols=(4, 5, 6), label_col=None)
S3DIS = dict(n_cols=6, xyz_cols=(0, 1, 2), rgb_cols=(3, 4, 5), label_col=None)
LABELS = dict(n_cols=1, xyz_cols=None, rgb_cols=None, label_col=0)


def _coord(rng, span=50.0, digits=3):
    return f'{rng.uniform(-span, span):.{digits}f}'


def sema_line(rng, span=50.0, digits=3, pad=0):
    """one `x y z intensity r g b` line; pad: that many leading zeros on the intensity (it is validated and dropped)."""
    xyz = [_coord(rng, span, digits) for _ in range(3)]
    return ' '.join(xyz + ['0' * pad + str(rng.randint(-2000, 2000))] + [str(rng.randint(0, 255)) for _ in range(3)])


def sema_text(seed, n, eol='\n', last_eol=True, **kw):
    rng = random.Random(seed)
    text = eol.join(sema_line(rng, **kw) for _ in range(n))
    return (text + eol if last_eol and n else text).encode()


def _long_line(rng):
    """a valid line of 40 ... 200 bytes: leading zeros in front of every field, many in front of the intensity"""
    f = sema_line(rng, digits=rng.randint(0, 9)).split(' ')
    out = []
    for k, t in enumerate(f):
        sign = t[0] if t[0] == '-' else ''
        out.append(sign + '0' * rng.randint(0, 130 if k == 3 else 3) + t[len(sign):])
    return ' '.join(out)


def _edge_text(seed, edge, shift, tail_lines=6):
    """lines of which one ends so that its '\\n' stands at byte edge - 1 + shift (shift 0: the last byte in front of the edge, 1: the
    first byte behind it); shift 'token': the x field of a line straddles the edge instead."""
    rng = random.Random(seed)
    lines, size = [], 0
    while True:
        line = _long_line(rng)
        if size + len(line) + 1 > edge - 260:
            break
        lines.append(line)
        size += len(line) + 1
    if shift == 'token':
        target = edge - 3                      # the next line starts 3 bytes in front of the edge: `-12.345` lies across it
    else:
        target = edge + shift                  # bytes up to and including the '\n'
    filler = sema_line(rng)
    pad = target - size - (len(filler) + 1)
    assert 0 <= pad <= 450
    f = filler.split(' ')
    sign = '-' if f[3][0] == '-' else ''
    f[3] = sign + '0' * pad + f[3][len(sign):]
    lines.append(' '.join(f))
    assert size + len(lines[-1]) + 1 == target
    lines += ['-12.3456 ' + sema_line(rng).split(' ', 1)[1]] + [_long_line(rng) for _ in range(tail_lines)]
    return ('\n'.join(lines) + '\n').encode()


# the last six digits of the 22 behind the point are zeros: pandas keeps 17 digits of a token, leading zeros included, and drops
# what follows, so its value is the correctly rounded one only while every non-zero digit is among the first 17
TOKEN_ROWS = ['0 -0 -0.000', '.5 5. +1.5', '000.25 123456789.012345 -0.0000000123456789000000', '-.5 +0 -5.',
              '999999999999999 0.000000000000001 +0000000000000001.5', '0.1 0.7 -0.3']
# inside the grammar, but with non-zero digits behind the 17th: float() is correctly rounded, pandas.read_csv is not
TOKEN_ROWS_PAST_PANDAS = ['-0.0000000000000000000001 +000000000000000000001.5 0.0000000000000012345678',
                          '0.0000000123456789012345 00000000000000000000012.75 -000000000000000000.5']


def parse_cases(layout=None):
    """[(name, dict(data, n_cols, xyz_cols, rgb_cols, label_col[, pandas=False: pandas.read_csv is not the judge of this one]))]"""
    layout = layout or DEFAULT_LAYOUT
    cases = []

    def add(name, data, spec=SEMA):
        cases.append((name, dict(spec, data=data)))
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        add(f'lines_{n}', sema_text(100 + n, n))
    add('no_final_newline', sema_text(1, 5, last_eol=False))
    add('crlf', sema_text(2, 70, eol='\r\n'))
    add('crlf_no_final', sema_text(3, 4, eol='\r\n', last_eol=False))
    blank = sema_text(4, 9).split(b'\n')
    add('blank_lines', b'\n'.join([b''] + blank[:3] + [b'', b''] + blank[3:6] + [b'\r'] + blank[6:9]) + b'\n\n\r\n\n')
    add('only_blank', b'\n\r\n\n')
    for k in (1, 3):                                # the first edge between two tiles of the index kernels, and a later one
        edge = k * layout['index_tile']
        add(f'tile_{k}_newline_last_byte', _edge_text(11 + k, edge, 0))
        add(f'tile_{k}_newline_first_byte', _edge_text(12 + k, edge, 1))
        add(f'tile_{k}_token_across', _edge_text(13 + k, edge, 'token'))
    longest = '1.5 2.5 3.5 {}7 1 2 3'
    add('max_line_exact', (longest.format('0' * (layout['max_line'] - len(longest) + 2)) + '\n' + sema_text(5, 2).decode()).encode())
    add('tokens', ('\n'.join(f'{r} 0 1 2 3' for r in TOKEN_ROWS) + '\n').encode())
    add('tokens_past_pandas', ('\n'.join(f'{r} 0 1 2 3' for r in TOKEN_ROWS_PAST_PANDAS) + '\n').encode())
    cases[-1][1]['pandas'] = False
    add('colours', b'1 2 3 0 0 255 12.0\n4 5 6 0 000255 -0 +7.000\n')
    add('s3dis_room', ('\n'.join(' '.join(sema_line(random.Random(60 + i)).split(' ')[:3] + ['10', '200', '30.000000'])
                                 for i in range(40)) + '\n').encode(), S3DIS)
    add('labels', ('\n'.join(str(random.Random(7).randint(0, 8)) for _ in range(33)) + '\n').encode(), LABELS)
    add('digits_6_9', sema_text(8, 50, digits=9, span=999.0))
    return cases


def refusal_cases(layout=None):
    """[(name, dict(data, ..., error=(code, line, offset)))]: a good line, the refused line, a good line."""
    layout = layout or DEFAULT_LAYOUT
    good = sema_text(21, 1).decode()               # (with its '\n')
    base = '1.25 -2.5 3 17 10 20 30'
    cases = []

    def add(name, bad, code, at, spec=SEMA, good=good):
        """at: the offset inside the refused line"""
        cases.append((name, dict(spec, data=(good + bad + '\n' + good).encode(), error=(code, 1, len(good) + at))))
    add('digits_16', '1.25 1234567.890123456 3 17 10 20 30', TOKEN, 5)
    add('fraction_23', '1.25 -2.5 0.00000000000000000000001 17 10 20 30', TOKEN, 10)
    add('exponent', '1.25 1e-3 3 17 10 20 30', BYTE, 6)
    add('nan', '1.25 -2.5 nan 17 10 20 30', BYTE, 10)
    add('fields_6', '1.25 -2.5 3 17 10 20', FIELDS, 20)
    add('fields_8', base + ' 40', FIELDS, len(base) + 1)
    add('double_space', '1.25  -2.5 3 17 10 20 30', EMPTY, 5)
    add('trailing_space', base + ' ', EMPTY, len(base) + 1)
    add('leading_space', ' ' + base, EMPTY, 0)
    add('byte_0x10', '1.25 -2.5 3 1\x107 10 20 30', BYTE, 13)
    add('lone_cr', '1.25 -2.5 3\r 17 10 20 30', BYTE, 11)
    add('two_points', '1.2.5 -2.5 3 17 10 20 30', TOKEN, 0)
    add('sign_inside', '1.25 2-5 3 17 10 20 30', TOKEN, 5)
    add('no_digit', '1.25 -. 3 17 10 20 30', TOKEN, 5)
    add('colour_256', '1.25 -2.5 3 17 256 20 30', RANGE, 15)
    add('colour_negative', '1.25 -2.5 3 17 10 -1 30', RANGE, 18)
    add('colour_fraction', '1.25 -2.5 3 17 10 20 3.5', RANGE, 21)
    add('label_300', '300', RANGE, 0, LABELS, '3\n')
    add('too_long', '1.25 -2.5 3 ' + '0' * layout['max_line'] + '17 10 20 30', LONG, layout['max_line'])
    return cases


def carry_cases():
    """[(name, dict(data, ..., rows, blocks))]: the block sizes put the end of the first block at every byte of line 2 (its
    terminator included), and a few blocks smaller than a line."""
    cases = []
    for name, eol, last in (('carry_lf', '\n', True), ('carry_crlf_open', '\r\n', False)):
        data = sema_text(31, 7, eol=eol, last_eol=last)
        first = data.index(b'\n', data.index(b'\n') + 1) + 1            # line 2 starts here
        end = data.index(b'\n', first) + 1
        cases.append((name, dict(SEMA, data=data, rows=3, blocks=[1, 7, 16] + list(range(first, end + 1)) + [len(data), len(data) + 5])))
    return cases


# ---- PARITY cases of the provider functions (run through the reference by tools/gen_cloud_text_golden.py) ----
def semantic3d_cases():
    """[(name, dict(data, labels | None, n_class, voxel_width, ver_batch))].  With labels, the reference drops the first line of
    data; label files have one line per line of data, and no label chunk the reference reads has exactly one row."""
    cases = []

    def add(name, seed, n, n_class, ver_batch, n_labels=None):
        rng = random.Random(seed)
        data = sema_text(seed, n, span=1.5, digits=4)
        labels = ('\n'.join(str(rng.randint(0, n_class)) for _ in range(n_labels or n)) + '\n').encode() if n_class else None
        cases.append((name, dict(data=data, labels=labels, n_class=n_class, voxel_width=0.5, ver_batch=ver_batch)))
    add('labelled_dividing', 41, 241, 8, 60)          # 240 points in chunks of 60; the label chunks read are 60 each
    add('labelled_not_dividing', 42, 200, 8, 64)      # 199 points: 64, 64, 64, 7; labels 64, 64, 64, 8
    add('labelled_one_line', 43, 1, 8, 10, 3)         # the only line is the header: no point
    add('unlabelled_dividing', 44, 192, 0, 64)
    add('unlabelled_not_dividing', 45, 150, 0, 64)
    add('unlabelled_one_chunk', 46, 30, 0, 1000)
    return cases


def interpolate_cases():
    """[(name, dict(data, xyz, labels, ver_batch))]: xyz = the float32 points of every third line, shifted a little."""
    cases = []
    for name, seed, n, ver_batch, hist in (('dividing', 51, 120, 40, False), ('not_dividing', 52, 131, 50, False),
                                           ('histograms', 53, 77, 500, True), ('one_chunk_exact', 54, 64, 64, False)):
        data = sema_text(seed, n, span=5.0)
        rng = np.random.default_rng(seed)
        pts = np.array([[float(t) for t in line.split(b' ')[:3]] for line in data.split(b'\n') if line], dtype=np.float32)
        xyz = np.ascontiguousarray(pts[::3] + rng.uniform(-0.01, 0.01, pts[::3].shape).astype(np.float32))
        labels = rng.integers(0, 9, (len(xyz), 9)).astype(np.uint32) if hist else rng.integers(0, 9, len(xyz)).astype(np.uint8)
        cases.append((name, dict(data=data, xyz=xyz, labels=labels, ver_batch=ver_batch)))
    return cases


def s3dis_cases():
    """[(name, dict(room, objects=[(file name, bytes)]))]: three objects in the order they are applied (the tests and the generator
    fix glob.glob's order to the sorted one); objects overlap, so the order shows.  Object points are room lines, every fourth
    moved by 0.001 along x (tests/test_cloud_text_restatement.py checks that no two room points are equidistant from one)."""
    rng = random.Random(61)
    room = [' '.join([f'{rng.uniform(0, 8):.3f}', f'{rng.uniform(0, 6):.3f}', f'{rng.uniform(0, 3):.3f}'] +
                     [f'{rng.randint(0, 255)}.000000' for _ in range(3)]) for _ in range(90)]
    objects = []
    for name, rows in (('chair_1', range(0, 40)), ('table_2', range(30, 70)), ('wall_1', range(60, 90, 2))):
        lines = []
        for r in rows:
            f = room[r].split(' ')
            if r % 4 == 0:
                f[0] = f'{float(f[0]) + 0.001:.3f}'
            lines.append(' '.join(f))
        objects.append((name + '.txt', ('\n'.join(lines) + '\n').encode()))
    return [('room_three_objects', dict(room=('\n'.join(room) + '\n').encode(), objects=objects))]
