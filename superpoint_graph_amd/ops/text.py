"""Raw cloud text parsed on the device, and the file reader that streams it there (csrc/spg_text.hip); result text formatted on the
device and error2ply's colours (csrc/spg_format.hip)."""
from __future__ import annotations

import ctypes

import torch

from .._lib import check, lib
from ._core import _int_vec, _on_gpu, _ptr, _req, _stream, _workspace


# --------------------------------------------------------------------------------------------------
# raw cloud text (csrc/spg_text.hip; pandas.read_csv in the reference's partition/provider.py): DESIGN.md section 4.11i
# --------------------------------------------------------------------------------------------------
TEXT_MAX_COLS = 16
TEXT_ERRORS = {1: 'the wrong number of fields', 2: 'an empty field (a leading, trailing or double space)',
               3: 'a byte that is not part of a number', 4: 'a field outside the number grammar ([+-]digits[.digits], at most 15 '
               'digits, at most 22 behind the point, no exponent)', 5: 'a colour or label that is not a whole number in [0, 255]',
               6: 'a line longer than the cap'}


class CloudTextError(ValueError):
    """A line outside the contract of parse_cloud_text.  line: the index of the first refused line among the non-blank lines,
    offset: the byte the code points at (both counted from the start of the buffer, or of the file in CloudTextReader),
    code: a key of TEXT_ERRORS, refused: how many lines of the buffer were refused."""

    def __init__(self, line, code, offset, refused, source=''):
        self.line, self.code, self.offset, self.refused = int(line), int(code), int(offset), int(refused)
        super().__init__(f'cloud text{" " + source if source else ""}: line {self.line} (non-blank lines counted from 0), byte '
                         f'{self.offset}: {TEXT_ERRORS.get(self.code, "refused")} [code {self.code}]; {self.refused} line(s) refused')


def text_layout():
    """{'index_tile', 'max_line'} of csrc/spg_text.hip in bytes (spg_text_debug_layout; host only)."""
    L = lib()
    return {'index_tile': int(L.spg_text_debug_layout(0)), 'max_line': int(L.spg_text_debug_layout(1))}


def _text_roles(n_cols, xyz_cols, rgb_cols, label_col):
    n_cols = int(n_cols)
    if not 1 <= n_cols <= TEXT_MAX_COLS:
        raise ValueError(f'parse_cloud_text: 1 <= n_cols <= {TEXT_MAX_COLS} expected, got {n_cols}')
    roles = [-1] * n_cols
    picks = []
    for name, cols, first in (('xyz_cols', xyz_cols, 0), ('rgb_cols', rgb_cols, 3)):
        if cols is not None:
            cols = [int(c) for c in cols]
            if len(cols) != 3:
                raise ValueError(f'parse_cloud_text: {name} names three columns')
            picks += [(c, first + k) for k, c in enumerate(cols)]
    if label_col is not None:
        picks.append((int(label_col), 6))
    if not picks:
        raise ValueError('parse_cloud_text: no column selected')
    for c, r in picks:
        if not 0 <= c < n_cols or roles[c] != -1:
            raise ValueError(f'parse_cloud_text: column {c} is outside 0 ... {n_cols - 1} or selected twice')
        roles[c] = r
    return (ctypes.c_int * n_cols)(*roles)


def parse_cloud_text(text_u8, n_cols, xyz_cols=(0, 1, 2), rgb_cols=None, label_col=None, final_block=True, line_base=0, byte_base=0,
                     source=''):
    """The lines of a text cloud (`x y z i r g b` of Semantic3D, `x y z r g b` of S3DIS, one label per line) parsed on the device:
    text_u8 uint8 [n_bytes] on the GPU -> (xyz f32 [n, 3] | None, rgb u8 [n, 3] | None, label u8 [n] | None, n, consumed).
    n_cols fields per line, separated by exactly one space; a line ends at '\\n' (one '\\r' in front belongs to it), empty lines are
    skipped.  consumed: the bytes up to and including the last complete line; with final_block an unterminated last line counts
    and consumed = n_bytes, without it the caller carries text_u8[consumed:] in front of the next block.
    Values: the digits as an integer over a power of ten in float64, rounded once to float32 (= np.float32(float(token)), what
    pandas.read_csv returns on this grammar); zeros are +0.0; rgb / label are whole numbers in [0, 255].  Everything else raises
    CloudTextError (a ValueError) that names the first refused line, its byte and the reason (include/spg_hip.h).
    Two host synchronisations: the line count, which sizes the outputs, and the error record behind the parse.
    line_base / byte_base / source only shift and label what an error reports."""
    _req(text_u8, torch.uint8, 'text_u8')
    if text_u8.dim() != 1:
        raise ValueError('parse_cloud_text: text_u8 must be one-dimensional')
    roles = _text_roles(n_cols, xyz_cols, rgb_cols, label_col)
    if text_u8.data_ptr() % 16:
        text_u8 = text_u8.clone()                 # (a slice: the 16-byte loads want the allocator's alignment)
    L, dev, st = lib(), text_u8.device, _stream()
    nb = int(text_u8.numel())
    ws = _workspace(L.spg_text_workspace_bytes, nb, dev=dev)
    head = torch.empty(2, dtype=torch.int64, device=dev)
    check(L.spg_text_index(_ptr(text_u8), nb, int(bool(final_block)), _ptr(head), _ptr(ws), ws.numel(), st), 'spg_text_index')
    n, consumed = (int(v) for v in head.tolist())
    line_start = torch.empty(n, dtype=torch.int64, device=dev)
    check(L.spg_text_lines(_ptr(text_u8), nb, n, _ptr(line_start), _ptr(ws), ws.numel(), st), 'spg_text_lines')
    xyz = torch.empty(n, 3, dtype=torch.float32, device=dev) if xyz_cols is not None else None
    rgb = torch.empty(n, 3, dtype=torch.uint8, device=dev) if rgb_cols is not None else None
    label = torch.empty(n, dtype=torch.uint8, device=dev) if label_col is not None else None
    error = torch.empty(4, dtype=torch.int64, device=dev)
    check(L.spg_text_parse(_ptr(text_u8), nb, _ptr(line_start), n, int(n_cols), roles, _ptr(xyz), _ptr(rgb), _ptr(label), _ptr(error),
                           st), 'spg_text_parse')
    first, code, where, refused = error.tolist()
    if refused:
        raise CloudTextError(line_base + first, code, byte_base + where, refused, source)
    return xyz, rgb, label, n, consumed


class CloudTextReader:
    """Iterates over a text cloud file in device batches of exactly `rows` lines (fewer in the last): (xyz, rgb, label) as
    parse_cloud_text returns them.  The file is read block_bytes at a time into one page-locked buffer and uploaded from there;
    the unfinished last line of a block is carried in front of the next, so the batches do not depend on block_bytes and a
    cloud larger than a block streams through.  Nothing is parsed on the host.  skip_lines: that many leading (non-blank) lines
    are parsed and dropped (the header line pandas consumes in the reference's read_semantic3d_format)."""

    def __init__(self, path, n_cols, xyz_cols=(0, 1, 2), rgb_cols=None, label_col=None, rows=1 << 20, block_bytes=1 << 26,
                 skip_lines=0, device=None):
        if int(rows) < 1 or int(block_bytes) < 1 or int(skip_lines) < 0:
            raise ValueError('CloudTextReader: rows >= 1, block_bytes >= 1 and skip_lines >= 0 expected')
        _text_roles(n_cols, xyz_cols, rgb_cols, label_col)
        self.path, self.n_cols, self.cols = path, int(n_cols), (xyz_cols, rgb_cols, label_col)
        self.rows, self.block_bytes, self.skip_lines = int(rows), int(block_bytes), int(skip_lines)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)

    def __iter__(self):
        max_line = text_layout()['max_line']
        pinned = torch.empty(self.block_bytes + max_line + 2, dtype=torch.uint8).pin_memory()
        host = pinned.numpy()
        carry, lines, offset, skip, held = 0, 0, 0, self.skip_lines, None
        with open(self.path, 'rb', buffering=0) as f:
            final = False
            while not final:
                got = 0
                while got < self.block_bytes:
                    r = f.readinto(memoryview(host)[carry + got:carry + self.block_bytes])
                    if not r:
                        final = True
                        break
                    got += r
                total = carry + got
                # (parse_cloud_text synchronises behind this copy, so the buffer is free again when it returns)
                text = pinned[:total].to(self.device, non_blocking=True)
                xyz, rgb, label, n, consumed = parse_cloud_text(text, self.n_cols, *self.cols, final_block=final,
                                                                line_base=lines, byte_base=offset, source=str(self.path))
                carry = total - consumed
                if carry > max_line + 2:
                    raise CloudTextError(lines + n, 6, offset + consumed + max_line, 1, str(self.path))
                host[:carry] = host[consumed:total].copy()
                lines, offset = lines + n, offset + consumed
                new = [None if t is None else t[min(skip, n):] for t in (xyz, rgb, label)]
                skip -= min(skip, n)
                held = new if held is None else [None if a is None else torch.cat((a, b)) for a, b in zip(held, new)]
                count = next(int(t.shape[0]) for t in held if t is not None)
                while count >= self.rows:
                    yield tuple(None if t is None else t[:self.rows] for t in held)
                    held = [None if t is None else t[self.rows:] for t in held]
                    count -= self.rows
        if held is not None and next(int(t.shape[0]) for t in held if t is not None) > 0:
            yield tuple(held)


# --------------------------------------------------------------------------------------------------
# result text (csrc/spg_format.hip; numpy.savetxt and plyfile's text writer in the reference): DESIGN.md section 4.11k
# --------------------------------------------------------------------------------------------------
FORMAT_KINDS = {torch.uint8: 0, torch.int32: 1, torch.uint32: 2, torch.int64: 3, torch.float32: 4}      # SPG_FORMAT_* of include/spg_hip.h
FORMAT_MAX_FIELD = {torch.uint8: 3, torch.int32: 11, torch.uint32: 10, torch.int64: 20, torch.float32: 24}      # bytes of the longest field


def _format_columns(columns):
    """columns -> (the 1-D views, n_rows): an entry is a device tensor [n] (any stride >= 0, e.g. a column of a matrix) or a
    contiguous [n, k], which stands for its k columns."""
    flat = []
    for i, t in enumerate(columns):
        name = f'columns[{i}]'
        _on_gpu(t, name)
        if t.dtype not in FORMAT_KINDS:
            raise TypeError(f'{name} must be uint8, int32, uint32, int64 or float32, got {t.dtype}')
        if t.dim() == 2:
            _req(t, None, name)
            flat += [t[:, j] for j in range(t.shape[1])]
        elif t.dim() == 1:
            _req(t[:1], None, name)                                    # (the device test; the stride is the column's own)
            if t.stride(0) < 0:
                raise ValueError(f'{name} must not have a negative stride')
            flat.append(t)
        else:
            raise ValueError(f'{name} must be [n] or [n, k], got {tuple(t.shape)}')
    if not 1 <= len(flat) <= TEXT_MAX_COLS:
        raise ValueError(f'format_table: 1 ... {TEXT_MAX_COLS} columns expected, got {len(flat)}')
    n = int(flat[0].shape[0])
    if any(int(t.shape[0]) != n for t in flat):
        raise ValueError(f'format_table: columns of different lengths {[int(t.shape[0]) for t in flat]}')
    return flat, n


def format_table_capacity(columns):
    """An upper bound of the bytes format_table writes for these columns (every field at its longest)."""
    flat, n = _format_columns(columns)
    return n * sum(FORMAT_MAX_FIELD[t.dtype] + 1 for t in flat)


def format_table(columns, out=None):
    """A table as text, formatted on the device: columns (at most 16 once [n, k] entries are expanded, see _format_columns) ->
    (bytes uint8 [total] on the device, row_start int64 [n + 1]): row r is bytes[row_start[r]:row_start[r + 1]], its fields joined
    by one space and ended by '\n'.  uint8 / int32 / uint32 / int64 fields are '%d', float32 fields are Python's
    '%.18g' % float(v) for every bit pattern -- the text numpy.savetxt writes with those formats (include/spg_hip.h).
    out: a uint8 device buffer to write into (its first `total` bytes are returned as a view); one too small raises
    RuntimeError before anything is written.  One host synchronisation: the total, which sizes the output."""
    flat, n = _format_columns(columns)
    if out is not None:
        _req(out, torch.uint8, 'out')
        if out.dim() != 1 or out.data_ptr() % 8:
            raise ValueError('format_table: out must be one-dimensional and 8-byte aligned')
    L, dev, st = lib(), flat[0].device, _stream()
    nc = len(flat)
    ptrs = (ctypes.c_void_p * nc)(*[t.data_ptr() for t in flat])
    kinds = (ctypes.c_int * nc)(*[FORMAT_KINDS[t.dtype] for t in flat])
    strides = (ctypes.c_long * nc)(*[int(t.stride(0)) for t in flat])
    ws = _workspace(L.spg_format_workspace_bytes, n, nc, dev=dev)
    row_start = torch.empty(n + 1, dtype=torch.int64, device=dev)
    check(L.spg_format_measure(ptrs, kinds, strides, nc, n, _ptr(row_start), _ptr(ws), ws.numel(), st), 'spg_format_measure')
    total = int(row_start[n])
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=dev)
    check(L.spg_format_write(ptrs, kinds, strides, nc, n, _ptr(row_start), total, _ptr(out), int(out.numel()), st), 'spg_format_write')
    return out[:total], row_start


def error_colours(rgb, labels, prediction):
    """error2ply's colours (partition/provider.py:73-98) on the device: rgb uint8 [n, 3], labels / prediction integer [n] ->
    uint8 [n, 3], green hue where label == prediction or label == 0 and red elsewhere, saturation + 0.3 and value + 0.1 capped
    at 1; float64 in colorsys's operation order, equal to the reference's Python loop for every input."""
    _req(rgb, torch.uint8, 'rgb')
    if rgb.dim() != 2 or rgb.shape[1] != 3:
        raise ValueError(f'error_colours: rgb must be [n, 3], got {tuple(rgb.shape)}')
    n = int(rgb.shape[0])
    labels, prediction = _int_vec(labels, n, torch.int64, 'labels'), _int_vec(prediction, n, torch.int64, 'prediction')
    out = torch.empty(n, 3, dtype=torch.uint8, device=rgb.device)
    check(lib().spg_error_colours(_ptr(rgb), _ptr(labels), _ptr(prediction), n, _ptr(out), _stream()), 'spg_error_colours')
    return out
