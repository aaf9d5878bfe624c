"""Plain Python restatement of the result text (csrc/spg_format.hip and the writers of partition/provider.py): the expected bytes
of a table built field by field with Python's % operator, the PLY header, and error2ply's colours by the reference's formula
with colorsys.  numpy and the standard library only; tests/test_result_text_restatement.py holds it to numpy.savetxt and to
the reference's results in tests/golden/result_text.npz."""
import colorsys

import numpy as np

PLY_NAMES = {'f4': 'float', 'u1': 'uchar', 'u4': 'uint', 'i4': 'int'}          # numpy dtype code -> the property type in the header


def field(v):
    """one value as the writers print it: '%.18g' of the exactly widened float32, '%d' of an integer"""
    return '%.18g' % float(v) if isinstance(v, (np.floating, float)) else '%d' % int(v)


def table_rows(columns):
    """columns: 1-D arrays of one length -> the lines (bytes, each ended by a newline)"""
    lists = [c.tolist() if c.dtype.kind in 'iu' else [float(v) for v in c] for c in columns]
    fmts = ['%d' if c.dtype.kind in 'iu' else '%.18g' for c in columns]
    return [(' '.join(f % v for f, v in zip(fmts, row)) + '\n').encode('ascii') for row in zip(*lists)]


def table_bytes(columns):
    return b''.join(table_rows(columns))


def row_starts(columns):
    """int64 [n + 1]: the offset of every line and the total"""
    return np.concatenate(([0], np.cumsum([len(r) for r in table_rows(columns)], dtype=np.int64))).astype(np.int64)


def ply_header(elements):
    """elements: [(name, count, [(property, numpy dtype code), ...]), ...] -> the header plyfile writes for text=True"""
    lines = ['ply', 'format ascii 1.0']
    for name, count, props in elements:
        lines.append('element %s %d' % (name, count))
        lines += ['property %s %s' % (PLY_NAMES[code], prop) for prop, code in props]
    return ('\n'.join(lines) + '\nend_header\n').encode('ascii')


def ply_bytes(elements):
    """elements: [(name, [(property, 1-D array), ...]), ...] -> the whole ASCII PLY file"""
    head = ply_header([(name, len(props[0][1]), [(p, a.dtype.str[1:]) for p, a in props]) for name, props in elements])
    return head + b''.join(table_bytes([a for _, a in props]) for _, props in elements)


def error_colours(rgb, labels, prediction):
    """error2ply's colours: rgb uint8 [n, 3], labels / prediction [n] -> uint8 [n, 3]"""
    color_rgb = rgb / 255
    for i in range(len(labels)):
        hsv = list(colorsys.rgb_to_hsv(color_rgb[i, 0], color_rgb[i, 1], color_rgb[i, 2]))
        hsv[0] = 0.333333 if labels[i] == prediction[i] or labels[i] == 0 else 0
        hsv[1] = min(1, hsv[1] + 0.3)
        hsv[2] = min(1, hsv[2] + 0.1)
        color_rgb[i, :] = list(colorsys.hsv_to_rgb(hsv[0], hsv[1], hsv[2]))
    return np.array(color_rgb * 255, dtype='u1')
