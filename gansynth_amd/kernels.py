"""Tensor-level wrappers over the C ABI (one method per kernel entry point).

Inputs/outputs are torch CUDA(HIP) tensors; torch only supplies device memory and the
current stream.  4-D activations are logical NCHW with channels-last strides, which is the
[n][h][w][c] layout the kernels expect.  Every method launches HIP kernels from
libgansynth_hip.so -- nothing here computes with torch ops.

The autograd layer (functional.py) talks to the module-level `K` object; tests may swap it for
an emulation to check the autograd algebra on CPU, the product never does.
"""
import contextlib
import ctypes
import math
import os

import numpy as np
import torch

from . import config
from . import _lib
from ._lib import GS_BF16, GS_F32

CL = torch.channels_last


def _dt(t):
    if t.dtype == torch.float32:
        return GS_F32
    if t.dtype == torch.bfloat16:
        return GS_BF16
    raise TypeError(f"unsupported activation dtype {t.dtype}")


def _act(x):
    """Make an activation tensor kernel-ready (channels-last for 4-D, contiguous otherwise)."""
    if x.dim() == 4:
        return x if x.is_contiguous(memory_format=CL) else x.contiguous(memory_format=CL)
    return x if x.is_contiguous() else x.contiguous()


def _f32c(t):
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.is_contiguous() else t.contiguous()


def _empty_like_act(shape, ref):
    if len(shape) == 4:
        return torch.empty(shape, dtype=ref.dtype, device=ref.device, memory_format=CL)
    return torch.empty(shape, dtype=ref.dtype, device=ref.device)


# 1-bit leaky-relu masks (include/gansynth_hip.h, GS_ACT_WRITE_BITS / GS_ACT_LRELU_BITS): a bf16 leaky-relu conv output that a later masked
# data-gradient launch will read only for its signs carries those signs behind it in the same allocation -- numel values, then numel / 8 bytes --
# and the masked launches read 1/16 of the bytes.  A tensor "has bits" when its storage is exactly that long: whoever allocated it here wrote them.
_MASK_BITS = not config.flag("GS_NO_MASK_BITS")


def _empty_act_with_bits(shape, ref):
    n, c, h, w = shape
    numel = n * c * h * w
    flat = torch.empty((numel + numel // 16,), dtype=ref.dtype, device=ref.device)
    return flat[:numel].view(n, h, w, c).permute(0, 3, 1, 2)


def _bits_wanted(ref, co, act):
    return _MASK_BITS and act == _lib.ACT_LRELU and ref.dtype == torch.bfloat16 and co % 32 == 0


def _has_bits(t):
    return (_MASK_BITS and t.dtype == torch.bfloat16 and t.dim() == 4 and t.shape[1] % 32 == 0 and t.storage_offset() == 0
            and t.untyped_storage().nbytes() == t.numel() * 2 + t.numel() // 8)


def _mask_act(mask, mask_act):
    return _lib.ACT_LRELU_BITS if (mask_act == _lib.ACT_LRELU and _has_bits(mask)) else int(mask_act)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_POISON = config.flag("GS_DEBUG_POISON_WS")   # debugging: workspaces start as NaN bit patterns, so that a
                                                                     # kernel reading workspace it never wrote shows up as NaN


def _ws(nbytes, device):
    if _POISON:
        return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device=device)
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _rows_cols(x):
    """(rows, channels) of a channels-last activation: rows = n*h*w for 4-D, b for 2-D."""
    if x.dim() == 4:
        n, c, h, w = x.shape
        return n * h * w, c
    return x.shape[0], x.shape[1]


def _note_table(channels, table, rows, length, total):
    """The checked, sorted rows of `table` as a ctypes array of the note struct of `channels` (1 or 2)."""
    name, gains, note = (("note_mix", ("gain",), _lib.GsMixNote) if channels == 1 else
                         ("note_mix_stereo", ("gain_l", "gain_r"), _lib.GsMixNoteStereo))   # (GsMixNoteStereo.reserved stays 0)
    checked = _checked_notes(name, table, rows, length, total, gains)
    return (note * len(checked))(*[note(*row) for row in checked])


def note_mix_table(table, rows, length, total):
    """The host side of note_mix: validates `table` -- (onset, hold, release, row, gain) per note -- against the waves' shape and the
    clip length, sorts it by (onset, position) and returns the rows as a ctypes array of GsMixNote.  ValueError by note index and
    field name.  (A note may run past `total`: it is clipped there.)"""
    return _note_table(1, table, rows, length, total)


def note_mix_stereo_table(table, rows, length, total):
    """The host side of note_mix_stereo: note_mix_table's checks and order for rows (onset, hold, release, row, gain_l, gain_r), as a
    ctypes array of GsMixNoteStereo."""
    return _note_table(2, table, rows, length, total)


def note_mix_curves_table(table, points, first, rows, length, total):
    """The host side of note_mix_curves: note_mix_table's checks and order for rows (onset, hold, release, row, gain, curve), and the
    curves -- `points`: rows (pos, v_l, v_r); `first`: len(curves) + 1 integers, curve p owning points[first[p]:first[p + 1]] -- checked:
    `first` non-decreasing from 0 to len(points) with every range non-empty, positions integers strictly increasing within a curve, values
    finite, every note's `curve` in range.  ValueError by index and field name.  -> (ctypes arrays of GsMixNoteCurve, GsCurvePoint and
    int32).  Needs no device."""
    what = "note_mix_curves"
    fields = ("onset", "hold", "release", "row", "gain", "curve")
    if len(table) == 0:
        raise ValueError(f"{what}: the table is empty")
    for i, entry in enumerate(table):
        if len(entry) != len(fields):
            raise ValueError(f"{what}: note {i} has {len(entry)} fields, not ({', '.join(fields)})")
    first = list(first)
    for p, v in enumerate(first):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
            raise ValueError(f"{what}: first[{p}] must be an integer (got {v!r})")
    if len(first) < 2 or first[0] != 0 or first[-1] != len(points):
        raise ValueError(f"{what}: first must run from 0 to len(points) = {len(points)} over at least one curve (got {first})")
    n_curves = len(first) - 1
    for p in range(n_curves):
        if not first[p] < first[p + 1]:
            raise ValueError(f"{what}: curve {p} has no point (first[{p}] = {first[p]}, first[{p + 1}] = {first[p + 1]})")
    curve_of = [p for p in range(n_curves) for _ in range(first[p], first[p + 1])]
    for j, point in enumerate(points):
        if len(point) != 3:
            raise ValueError(f"{what}: point {j} has {len(point)} fields, not (pos, v_l, v_r)")
        pos = point[0]
        if not isinstance(pos, (int, np.integer)) or isinstance(pos, bool):
            raise ValueError(f"{what}: point {j} field 'pos' must be an integer (got {pos!r})")
        if j > first[curve_of[j]] and not points[j - 1][0] < pos:
            raise ValueError(f"{what}: point {j} field 'pos' = {pos} does not come after point {j - 1}'s {points[j - 1][0]} in curve {curve_of[j]}")
        for name, v in zip(("v_l", "v_r"), point[1:]):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not np.isfinite(v):
                raise ValueError(f"{what}: point {j} field '{name}' must be a finite number (got {v!r})")
    for i, entry in enumerate(table):
        curve = entry[5]
        if not isinstance(curve, (int, np.integer)) or isinstance(curve, bool):
            raise ValueError(f"{what}: note {i} field 'curve' must be an integer (got {curve!r})")
        if not 0 <= curve < n_curves:
            raise ValueError(f"{what}: note {i} field 'curve' = {curve} is outside [0, {n_curves})")
    checked = _checked_notes(what, [tuple(entry[:5]) for entry in table], rows, length, total, ("gain",))
    order = sorted(range(len(table)), key=lambda i: (int(table[i][0]), i))   # (_checked_notes' order)
    notes = (_lib.GsMixNoteCurve * len(checked))(*[_lib.GsMixNoteCurve(*row, int(table[i][5]), 0) for row, i in zip(checked, order)])
    pts = (_lib.GsCurvePoint * len(points))(*[_lib.GsCurvePoint(int(pos), float(v_l), float(v_r)) for pos, v_l, v_r in points])
    return notes, pts, (ctypes.c_int32 * len(first))(*[int(v) for v in first])


def note_warp_table(warp_notes, points, first, rows, length):
    """The host side of note_warp: `warp_notes` -- rows (src_row, dst_row, onset, count, curve) -- and the ratio curves -- `points`: rows
    (pos, ratio, cum); `first`: len(curves) + 1 integers, curve p owning points[first[p]:first[p + 1]] -- checked: rows inside [0, rows),
    no dst_row that is a src_row or the dst_row of another note, count in [1, length], onset >= 0, curve in range; `first` non-decreasing
    from 0 to len(points) with every range non-empty; positions integer-valued and strictly increasing within a curve, ratios in
    [0.25, 4], cum finite.  ValueError by index and field name.  -> (ctypes arrays of GsWarpNote, GsWarpPoint and int32).  Needs no
    device."""
    what = "note_warp"
    fields = ("src_row", "dst_row", "onset", "count", "curve")
    if len(warp_notes) == 0:
        raise ValueError(f"{what}: the table is empty")
    first = list(first)
    for p, v in enumerate(first):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
            raise ValueError(f"{what}: first[{p}] must be an integer (got {v!r})")
    if len(first) < 2 or first[0] != 0 or first[-1] != len(points):
        raise ValueError(f"{what}: first must run from 0 to len(points) = {len(points)} over at least one curve (got {first})")
    n_curves = len(first) - 1
    for p in range(n_curves):
        if not first[p] < first[p + 1]:
            raise ValueError(f"{what}: curve {p} has no point (first[{p}] = {first[p]}, first[{p + 1}] = {first[p + 1]})")
    for j, point in enumerate(points):
        if len(point) != 3:
            raise ValueError(f"{what}: point {j} has {len(point)} fields, not (pos, ratio, cum)")
    try:   # (a sequenced file can hold thousands of points: checked as arrays, reported by the first offender)
        values = np.array(points, dtype=np.float64).reshape(-1, 3)
    except (TypeError, ValueError):
        values = np.full((len(points), 3), np.nan)
        for j, point in enumerate(points):
            for k, v in enumerate(point):
                if not isinstance(v, bool) and isinstance(v, (int, float, np.floating, np.integer)):
                    values[j, k] = v
    pos, ratio = values[:, 0], values[:, 1]
    after = np.ones(len(points), dtype=bool)
    after[1:] = pos[1:] > pos[:-1]
    after[first[:-1]] = True                                   # a curve's first point follows nothing
    problems = [(~np.isfinite(values[:, k]), name, "must be a finite number") for k, name in enumerate(("pos", "ratio", "cum"))] + \
               [((pos != np.floor(pos)) | (np.abs(pos) > 2.0 ** 53), "pos", "must be a whole clip sample"),
                (~after, "pos", "does not come after the point before it in its curve"), (~((ratio >= 0.25) & (ratio <= 4.0)), "ratio", "is outside [0.25, 4]")]
    bad = [(int(np.argmax(mask)), name, why) for mask, name, why in problems if mask.any()]
    if bad:
        j, name, why = min(bad, key=lambda b: b[0])
        raise ValueError(f"{what}: point {j} field '{name}' {why} (got {points[j][('pos', 'ratio', 'cum').index(name)]!r})")
    sources = set()
    for i, entry in enumerate(warp_notes):
        if len(entry) != len(fields):
            raise ValueError(f"{what}: note {i} has {len(entry)} fields, not ({', '.join(fields)})")
        for name, v in zip(fields, entry):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
                raise ValueError(f"{what}: note {i} field '{name}' must be an integer (got {v!r})")
        src, dst, onset, count, curve = entry
        if not 0 <= src < rows:
            raise ValueError(f"{what}: note {i} field 'src_row' = {src} is outside [0, {rows})")
        if not 0 <= dst < rows:
            raise ValueError(f"{what}: note {i} field 'dst_row' = {dst} is outside [0, {rows})")
        if not 1 <= count <= length:
            raise ValueError(f"{what}: note {i} field 'count' = {count} is outside [1, {length}]")
        if not 0 <= onset < 2 ** 62:
            raise ValueError(f"{what}: note {i} field 'onset' = {onset} is negative (or beyond 2^62)")
        if not 0 <= curve < n_curves:
            raise ValueError(f"{what}: note {i} field 'curve' = {curve} is outside [0, {n_curves})")
        sources.add(int(src))
    written = set()
    for i, entry in enumerate(warp_notes):
        dst = int(entry[1])
        if dst in sources or dst in written:
            raise ValueError(f"{what}: note {i} field 'dst_row' = {dst} is the src_row or the dst_row of another note")
        written.add(dst)
    notes = (_lib.GsWarpNote * len(warp_notes))(*[_lib.GsWarpNote(*[int(v) for v in entry]) for entry in warp_notes])
    pts = (_lib.GsWarpPoint * len(points)).from_buffer_copy(np.ascontiguousarray(values).tobytes())
    return notes, pts, (ctypes.c_int32 * len(first))(*[int(v) for v in first])


def _sustain_ints(what, kind, i, fields, entry):
    if len(entry) != len(fields):
        raise ValueError(f"{what}: {kind} {i} has {len(entry)} fields, not ({', '.join(fields)})")
    for name, v in zip(fields, entry):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
            raise ValueError(f"{what}: {kind} {i} field '{name}' must be an integer (got {v!r})")


def loop_search_table(search_notes, rows, length, n_lags):
    """The host side of loop_search: `search_notes` -- rows (row, a, m_min, m_max, window) -- checked: row inside [0, rows), a >= 0,
    1 <= m_min <= m_max, window in [1, GS_SUSTAIN_MAX_WINDOW], a + m_max + window <= length and m_max - m_min + 1 <= n_lags (the
    row length of the scores).  ValueError by index and field name.  -> a ctypes array of GsLoopNote.  Needs no device."""
    what = "loop_search"
    fields = ("row", "a", "m_min", "m_max", "window")
    if len(search_notes) == 0:
        raise ValueError(f"{what}: the table is empty")
    for i, entry in enumerate(search_notes):
        _sustain_ints(what, "note", i, fields, entry)
        row, a, m_min, m_max, window = entry
        if not 0 <= row < rows:
            raise ValueError(f"{what}: note {i} field 'row' = {row} is outside [0, {rows})")
        if a < 0:
            raise ValueError(f"{what}: note {i} field 'a' = {a} is negative")
        if m_min < 1:
            raise ValueError(f"{what}: note {i} field 'm_min' = {m_min} is below 1")
        if m_max < m_min:
            raise ValueError(f"{what}: note {i} field 'm_max' = {m_max} is below m_min = {m_min}")
        if not 1 <= window <= _lib.SUSTAIN_MAX_WINDOW:
            raise ValueError(f"{what}: note {i} field 'window' = {window} is outside [1, {_lib.SUSTAIN_MAX_WINDOW}]")
        if a + m_max + window > length:
            raise ValueError(f"{what}: note {i} field 'm_max': a + m_max + window = {a + m_max + window} is beyond the length {length}")
        if m_max - m_min + 1 > n_lags:
            raise ValueError(f"{what}: note {i} field 'm_max': {m_max - m_min + 1} lags are more than the {n_lags} of a row of scores")
    return (_lib.GsLoopNote * len(search_notes))(*[_lib.GsLoopNote(*[int(v) for v in entry], 0) for entry in search_notes])


def note_sustain_table(jobs, rows, length):
    """The host side of note_sustain: `jobs` -- rows (src_row, dst_row, offset, count, a, m, xfade) -- checked: rows inside [0, rows), no
    dst_row that is a src_row or the dst_row of another job, count in [1, length], offset in [0, 2^62), a >= 0, m >= 1, xfade >= 0 and
    a + m + xfade <= length.  ValueError by index and field name.  -> a ctypes array of GsSustainJob.  Needs no device."""
    what = "note_sustain"
    fields = ("src_row", "dst_row", "offset", "count", "a", "m", "xfade")
    if len(jobs) == 0:
        raise ValueError(f"{what}: the table is empty")
    sources = set()
    for i, entry in enumerate(jobs):
        _sustain_ints(what, "job", i, fields, entry)
        src, dst, offset, count, a, m, xfade = entry
        if not 0 <= src < rows:
            raise ValueError(f"{what}: job {i} field 'src_row' = {src} is outside [0, {rows})")
        if not 0 <= dst < rows:
            raise ValueError(f"{what}: job {i} field 'dst_row' = {dst} is outside [0, {rows})")
        if not 0 <= offset < 2 ** 62:
            raise ValueError(f"{what}: job {i} field 'offset' = {offset} is negative (or beyond 2^62)")
        if not 1 <= count <= length:
            raise ValueError(f"{what}: job {i} field 'count' = {count} is outside [1, {length}]")
        if a < 0:
            raise ValueError(f"{what}: job {i} field 'a' = {a} is negative")
        if m < 1:
            raise ValueError(f"{what}: job {i} field 'm' = {m} is below 1")
        if xfade < 0:
            raise ValueError(f"{what}: job {i} field 'xfade' = {xfade} is negative")
        if a + m + xfade > length:
            raise ValueError(f"{what}: job {i} field 'xfade': a + m + xfade = {a + m + xfade} is beyond the length {length}")
        sources.add(int(src))
    written = set()
    for i, entry in enumerate(jobs):
        dst = int(entry[1])
        if dst in sources or dst in written:
            raise ValueError(f"{what}: job {i} field 'dst_row' = {dst} is the src_row or the dst_row of another job")
        written.add(dst)
    return (_lib.GsSustainJob * len(jobs))(*[_lib.GsSustainJob(*[int(v) for v in entry]) for entry in jobs])


def fft_convolve_shapes(x, impulse, dry, wet):
    """The host side of fft_convolve: -> (rows, n, ir_rows, m) of x ([n] or [rows, n], rows 1 or 2) and impulse ([m] or [ir_rows, m],
    ir_rows 1 or rows), both fp32.  ValueError by argument name; needs no device."""
    for name, t in (("x", x), ("impulse", impulse)):
        if not isinstance(t, torch.Tensor) or t.dim() not in (1, 2) or t.dtype != torch.float32 or t.numel() == 0:
            got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"fft_convolve: {name} must be a non-empty fp32 vector or [rows, samples] matrix (got {got})")
    rows, n = (1, int(x.shape[0])) if x.dim() == 1 else (int(x.shape[0]), int(x.shape[1]))
    ir_rows, m = (1, int(impulse.shape[0])) if impulse.dim() == 1 else (int(impulse.shape[0]), int(impulse.shape[1]))
    if rows > 2:
        raise ValueError(f"fft_convolve: x must have 1 or 2 rows -- a clip is mono or stereo (got {rows})")
    if ir_rows not in (1, rows):
        raise ValueError(f"fft_convolve: impulse must have 1 row or as many as x, {rows} (got {ir_rows})")
    if m > _lib.FFTCONV_MAX_TAPS:
        raise ValueError(f"fft_convolve: impulse has {m} taps, more than {_lib.FFTCONV_MAX_TAPS}")
    for name, v in (("dry", dry), ("wet", wet)):
        if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v):
            raise ValueError(f"fft_convolve: {name} must be a finite number (got {v!r})")
    return rows, n, ir_rows, m


def fft_convolve(x, impulse, dry, wet, normalize=True, want_pcm=False):
    """HipKernels.fft_convolve of the process-wide kernel object; the shapes are refused here, before a device is asked for."""
    fft_convolve_shapes(x, impulse, dry, wet)
    return get().fft_convolve(x, impulse, dry, wet, normalize=normalize, want_pcm=want_pcm)


def limit_shapes(x, pre_gain, ceiling, lookahead):
    """The host side of limit: -> (rows, n) of x ([n] or [rows, n] fp32, rows 1 or 2); pre_gain finite and > 0, ceiling in (0, 1] -- both
    as the fp32 values the kernel receives --, lookahead an integer number of samples in [1, LIMIT_MAX_LOOKAHEAD].  ValueError by argument
    name; needs no device."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2) or x.dtype != torch.float32 or x.numel() == 0:
        got = f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"limit: x must be a non-empty fp32 vector or [rows, samples] matrix (got {got})")
    rows, n = (1, int(x.shape[0])) if x.dim() == 1 else (int(x.shape[0]), int(x.shape[1]))
    if rows > 2:
        raise ValueError(f"limit: x must have 1 or 2 rows -- a clip is mono or stereo (got {rows})")
    for name, v in (("pre_gain", pre_gain), ("ceiling", ceiling)):
        if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v):
            raise ValueError(f"limit: {name} must be a finite number (got {v!r})")
    if not (pre_gain > 0 and math.isfinite(ctypes.c_float(pre_gain).value) and ctypes.c_float(pre_gain).value > 0):
        raise ValueError(f"limit: pre_gain must be positive and finite in fp32 (got {pre_gain!r})")
    if not 0 < ctypes.c_float(ceiling).value <= 1:
        raise ValueError(f"limit: ceiling must be in (0, 1] (got {ceiling!r})")
    if not isinstance(lookahead, (int, np.integer)) or isinstance(lookahead, bool) or not 1 <= lookahead <= _lib.LIMIT_MAX_LOOKAHEAD:
        raise ValueError(f"limit: lookahead must be an integer number of samples in [1, {_lib.LIMIT_MAX_LOOKAHEAD}] (got {lookahead!r})")
    return rows, n


def limit(x, pre_gain, ceiling, lookahead, want_pcm=False, envelope=None):
    """HipKernels.limit of the process-wide kernel object; the arguments are refused here, before a device is asked for."""
    rows, n = limit_shapes(x, pre_gain, ceiling, lookahead)
    if envelope is None:   # (the call it was)
        return get().limit(x, pre_gain, ceiling, lookahead, want_pcm=want_pcm)
    envelope_shape(envelope, n)
    return get().limit(x, pre_gain, ceiling, lookahead, want_pcm=want_pcm, envelope=envelope)


def envelope_shape(envelope, n):
    """limit's envelope: an fp32 vector of the clip's n samples (true_peak's first result).  ValueError; needs no device."""
    if not isinstance(envelope, torch.Tensor) or envelope.dtype != torch.float32 or tuple(envelope.shape) != (n,):
        got = f"{tuple(envelope.shape)} {envelope.dtype}" if isinstance(envelope, torch.Tensor) else type(envelope).__name__
        raise ValueError(f"limit: envelope must be an fp32 vector of the clip's {n} samples (got {got})")


def true_peak_shapes(x):
    """The host side of true_peak: -> (rows, n) of x ([n] or [rows, n] fp32, rows 1 or 2).  ValueError; needs no device."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2) or x.dtype != torch.float32 or x.numel() == 0:
        got = f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"true_peak: x must be a non-empty fp32 vector or [rows, samples] matrix (got {got})")
    rows, n = (1, int(x.shape[0])) if x.dim() == 1 else (int(x.shape[0]), int(x.shape[1]))
    if rows > 2:
        raise ValueError(f"true_peak: x must have 1 or 2 rows -- a clip is mono or stereo (got {rows})")
    return rows, n


def true_peak(x, want_envelope=True):
    """HipKernels.true_peak of the process-wide kernel object; the shape is refused here, before a device is asked for."""
    true_peak_shapes(x)
    return get().true_peak(x, want_envelope=want_envelope)


def _kmeans_matrix(what, name, t, cols=None):
    """x / centres of the k-means entries: a non-empty fp32 matrix (with `cols` columns); -> (rows, columns).  ValueError by argument name."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32 or t.numel() == 0 or (cols is not None and t.shape[1] != cols):
        got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
        want = "[rows, columns]" if cols is None else f"[rows, {cols}]"
        raise ValueError(f"{what}: {name} must be a non-empty fp32 {want} matrix (got {got})")
    return int(t.shape[0]), int(t.shape[1])


def _kmeans_vector(what, name, t, n, dtype):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (n,) or not t.is_contiguous():
        got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what}: {name} must be a contiguous {str(dtype).replace('torch.', '')} vector of {n} (got {got})")


def _kmeans_nk(what, n, k, d=1):
    if n > _lib.KMEANS_MAX_N:
        raise ValueError(f"{what}: x must have at most {_lib.KMEANS_MAX_N} rows (got {n})")
    if d > _lib.KMEANS_MAX_D:
        raise ValueError(f"{what}: x must have at most {_lib.KMEANS_MAX_D} columns (got {d})")
    if k > _lib.KMEANS_MAX_K:
        raise ValueError(f"{what}: centres must have at most {_lib.KMEANS_MAX_K} rows (got {k})")


def kmeans_assign_shapes(x, centres, labels=None):
    """The host side of kmeans_assign: -> (n, d, k) of x [n, d] and centres [k, d] (fp32, k <= KMEANS_MAX_K); labels, when given, a contiguous
    int32 vector of n.  ValueError by argument name; needs no device."""
    n, d = _kmeans_matrix("kmeans_assign", "x", x)
    k, _ = _kmeans_matrix("kmeans_assign", "centres", centres, d)
    _kmeans_nk("kmeans_assign", n, k, d)
    if labels is not None:
        _kmeans_vector("kmeans_assign", "labels", labels, n, torch.int32)
    return n, d, k


def kmeans_assign(x, centres, labels=None, want_dist=True, want_inertia=False):
    """HipKernels.kmeans_assign of the process-wide kernel object; the shapes are refused here, before a device is asked for."""
    kmeans_assign_shapes(x, centres, labels)
    return get().kmeans_assign(x, centres, labels=labels, want_dist=want_dist, want_inertia=want_inertia)


def kmeans_inertia_shapes(x, centres, labels):
    """The host side of kmeans_inertia: -> (n, d, k) of x [n, d], centres [k, d] (fp32) and labels (a contiguous int32 vector of n).  ValueError by
    argument name; needs no device."""
    n, d = _kmeans_matrix("kmeans_inertia", "x", x)
    k, _ = _kmeans_matrix("kmeans_inertia", "centres", centres, d)
    _kmeans_nk("kmeans_inertia", n, k, d)
    _kmeans_vector("kmeans_inertia", "labels", labels, n, torch.int32)
    return n, d, k


def kmeans_inertia(x, centres, labels):
    """HipKernels.kmeans_inertia of the process-wide kernel object; the shapes are refused here, before a device is asked for."""
    kmeans_inertia_shapes(x, centres, labels)
    return get().kmeans_inertia(x, centres, labels)


def kmeans_update_shapes(x, labels, centres):
    """The host side of kmeans_update: -> (n, d, k) of x [n, d], labels (a contiguous int32 vector of n) and centres [k, d] (fp32, contiguous:
    written in place).  ValueError by argument name; needs no device."""
    n, d = _kmeans_matrix("kmeans_update", "x", x)
    _kmeans_vector("kmeans_update", "labels", labels, n, torch.int32)
    k, _ = _kmeans_matrix("kmeans_update", "centres", centres, d)
    if not centres.is_contiguous():
        raise ValueError("kmeans_update: centres must be contiguous (it is written in place)")
    _kmeans_nk("kmeans_update", n, k, d)
    return n, d, k


def kmeans_update(x, labels, centres):
    """HipKernels.kmeans_update of the process-wide kernel object; the shapes are refused here, before a device is asked for."""
    kmeans_update_shapes(x, labels, centres)
    return get().kmeans_update(x, labels, centres)


def kmeans_mindist_shapes(x, centre, dist=None):
    """The host side of kmeans_mindist: -> (n, d) of x [n, d] and centre (a contiguous fp32 vector of d); dist, when given (the running minimum),
    a contiguous fp32 vector of n.  ValueError by argument name; needs no device."""
    n, d = _kmeans_matrix("kmeans_mindist", "x", x)
    _kmeans_vector("kmeans_mindist", "centre", centre, d, torch.float32)
    _kmeans_nk("kmeans_mindist", n, 1, d)
    if dist is not None:
        _kmeans_vector("kmeans_mindist", "dist", dist, n, torch.float32)
    return n, d


def kmeans_mindist(x, centre, dist=None):
    """HipKernels.kmeans_mindist of the process-wide kernel object; the shapes are refused here, before a device is asked for."""
    kmeans_mindist_shapes(x, centre, dist)
    return get().kmeans_mindist(x, centre, dist=dist)


def _knn_nm(what, names, n, m, d):
    for name, rows in zip(names, (n, m)):
        if rows > _lib.KMEANS_MAX_N:
            raise ValueError(f"{what}: {name} must have at most {_lib.KMEANS_MAX_N} rows (got {rows})")
    if d > _lib.KMEANS_MAX_D:
        raise ValueError(f"{what}: {names[0]} must have at most {_lib.KMEANS_MAX_D} columns (got {d})")


def knn_kth_shapes(a, b, k):
    """The host side of knn_kth: -> (n, m, d) of a [n, d] and b [m, d] (fp32; b may be a itself) and k in [1, KNN_MAX_K].  ValueError by argument
    name; needs no device."""
    n, d = _kmeans_matrix("knn_kth", "a", a)
    m, _ = _kmeans_matrix("knn_kth", "b", b, d)
    _knn_nm("knn_kth", ("a", "b"), n, m, d)
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= _lib.KNN_MAX_K:
        raise ValueError(f"knn_kth: k must be an integer in [1, {_lib.KNN_MAX_K}] (got {k!r})")
    return n, m, d


def knn_kth(a, b, k, exclude_diagonal=False):
    """HipKernels.knn_kth of the process-wide kernel object; the shapes are refused here, before a device is asked for."""
    knn_kth_shapes(a, b, k)
    return get().knn_kth(a, b, k, exclude_diagonal=exclude_diagonal)


def knn_within_shapes(q, ref, radius2):
    """The host side of knn_within: -> (n, m, d) of q [n, d], ref [m, d] (fp32) and radius2 (a contiguous fp32 vector of m).  ValueError by
    argument name; needs no device."""
    n, d = _kmeans_matrix("knn_within", "q", q)
    m, _ = _kmeans_matrix("knn_within", "ref", ref, d)
    _knn_nm("knn_within", ("q", "ref"), n, m, d)
    _kmeans_vector("knn_within", "radius2", radius2, m, torch.float32)
    return n, m, d


def knn_within(q, ref, radius2):
    """HipKernels.knn_within of the process-wide kernel object; the shapes are refused here, before a device is asked for."""
    knn_within_shapes(q, ref, radius2)
    return get().knn_within(q, ref, radius2)


def kid_sums_shapes(x, y, xi=None, yi=None):
    """The host side of kid_sums: -> (n, m, d, subsets, size) of x [n, d] and y [m, d] (fp32, at least 2 rows each) and the index lists xi, yi
    ([subsets, size] integers, numpy or torch, both or neither; (n, m, d, 0, 0) without).  ValueError by argument name; needs no device (lists
    that live on the device are read back for their range)."""
    n, d = _kmeans_matrix("kid_sums", "x", x)
    m, _ = _kmeans_matrix("kid_sums", "y", y, d)
    for name, rows in (("x", n), ("y", m)):
        if rows < 2:
            raise ValueError(f"kid_sums: {name} must have at least 2 rows (got {rows})")
        if rows > _lib.KID_MAX_ROWS:
            raise ValueError(f"kid_sums: {name} must have at most {_lib.KID_MAX_ROWS} rows (got {rows})")
    if d > _lib.KMEANS_MAX_D:
        raise ValueError(f"kid_sums: x must have at most {_lib.KMEANS_MAX_D} columns (got {d})")
    if xi is None and yi is None:
        return n, m, d, 0, 0
    shapes = []
    for name, t, rows in (("xi", xi, n), ("yi", yi, m)):
        integral = (isinstance(t, torch.Tensor) and t.dtype in (torch.int32, torch.int64)) or (isinstance(t, np.ndarray) and t.dtype.kind in "iu")
        if not integral or len(t.shape) != 2 or t.shape[0] < 1:
            got = "None" if t is None else f"{tuple(t.shape)} {t.dtype}" if hasattr(t, "shape") else type(t).__name__
            raise ValueError(f"kid_sums: {name} must be a [subsets, size] integer array or tensor with at least one subset (got {got})")
        if t.shape[1] < 2:
            raise ValueError(f"kid_sums: {name} holds subsets of size {t.shape[1]}: size must be at least 2")
        low, high = (int(t.min()), int(t.max()))
        if low < 0 or high >= rows:
            raise ValueError(f"kid_sums: {name} holds an index outside its set of {rows} rows ({low if low < 0 else high})")
        shapes.append(tuple(int(v) for v in t.shape))
    if shapes[0] != shapes[1]:
        raise ValueError(f"kid_sums: xi and yi differ in shape ({shapes[0]} and {shapes[1]})")
    subsets, size = shapes[0]
    if subsets > _lib.KID_MAX_SUBSETS:
        raise ValueError(f"kid_sums: xi holds {subsets} subsets, at most {_lib.KID_MAX_SUBSETS} go into one call")
    if size > min(n, m):
        raise ValueError(f"kid_sums: xi holds subsets of size {size}, above the smaller set's {min(n, m)} rows")
    return n, m, d, subsets, size


def kid_sums(x, y, xi=None, yi=None):
    """HipKernels.kid_sums of the process-wide kernel object; the shapes and the lists are refused here, before a device is asked for."""
    kid_sums_shapes(x, y, xi, yi)
    return get().kid_sums(x, y, xi, yi)


YIN_MAX_LAGS, YIN_MAX_WINDOW = 1024, 4096   # GS_YIN_MAX_LAGS, GS_YIN_MAX_WINDOW


def _yin_int(what, name, v):
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
        raise ValueError(f"{what}: {name} must be an integer (got {v!r})")
    return int(v)


def yin_frames(n, window, lags, hop):
    """gs_yin_frames restated on the host: (n - window - lags) // hop + 1 frames of a row of n samples; ValueError, by argument name, for what
    the entries refuse."""
    n, window, lags, hop = (_yin_int("yin", name, v) for name, v in (("n", n), ("window", window), ("lags", lags), ("hop", hop)))
    if not 4 <= lags <= YIN_MAX_LAGS:
        raise ValueError(f"yin: lags must be in [4, {YIN_MAX_LAGS}] (got {lags})")
    if not lags <= window <= YIN_MAX_WINDOW:
        raise ValueError(f"yin: window must be in [lags, {YIN_MAX_WINDOW}] (got {window}, lags {lags})")
    if hop < 1:
        raise ValueError(f"yin: hop must be positive (got {hop})")
    if n < window + lags:
        raise ValueError(f"yin: a row of {n} samples is shorter than window + lags = {window + lags}")
    return (n - window - lags) // hop + 1


def _yin_pick_args(what, lags, tau_min, threshold):
    lags, tau_min = _yin_int(what, "lags", lags), _yin_int(what, "tau_min", tau_min)
    if tau_min < 2:
        raise ValueError(f"{what}: tau_min must be at least 2 (got {tau_min})")
    if not tau_min + 2 <= lags <= YIN_MAX_LAGS:
        raise ValueError(f"{what}: lags must be in [tau_min + 2, {YIN_MAX_LAGS}] (got {lags}, tau_min {tau_min})")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.floating)) or not float(threshold) == float(threshold):
        raise ValueError(f"{what}: threshold must be a number (got {threshold!r})")


def yin_difference_shapes(x, window, lags, hop):
    """The host side of yin_difference: -> (rows, n, frames) of x [rows, n] (fp32).  ValueError by argument name; needs no device."""
    rows, n = _kmeans_matrix("yin_difference", "x", x)
    return rows, n, yin_frames(n, window, lags, hop)


def yin_difference(x, window, lags, hop):
    """HipKernels.yin_difference of the process-wide kernel object; the shapes are refused here, before a device is asked for."""
    yin_difference_shapes(x, window, lags, hop)
    return get().yin_difference(x, window, lags, hop)


def yin_pick_shapes(d, tau_min, threshold):
    """The host side of yin_pick: -> (rows, frames, lags) of d [rows, frames, lags] (fp32, contiguous).  ValueError by argument name; needs no
    device."""
    if not isinstance(d, torch.Tensor) or d.dim() != 3 or d.dtype != torch.float32 or 0 in d.shape or not d.is_contiguous():
        got = f"{tuple(d.shape)} {d.dtype}" if isinstance(d, torch.Tensor) else type(d).__name__
        raise ValueError(f"yin_pick: d must be a non-empty contiguous [rows, frames, lags] fp32 tensor (got {got})")
    _yin_pick_args("yin_pick", int(d.shape[2]), tau_min, threshold)
    return tuple(int(s) for s in d.shape)


def yin_pick(d, tau_min, threshold):
    """HipKernels.yin_pick of the process-wide kernel object; the shapes are refused here, before a device is asked for."""
    yin_pick_shapes(d, tau_min, threshold)
    return get().yin_pick(d, tau_min, threshold)


def yin_track_shapes(x, window, lags, hop, tau_min, threshold):
    """The host side of yin_track: -> (rows, n, frames) of x [rows, n] (fp32).  ValueError by argument name; needs no device."""
    rows, n = _kmeans_matrix("yin_track", "x", x)
    frames = yin_frames(n, window, lags, hop)
    _yin_pick_args("yin_track", lags, tau_min, threshold)
    return rows, n, frames


def yin_track(x, window, lags, hop, tau_min, threshold):
    """HipKernels.yin_track of the process-wide kernel object; the shapes are refused here, before a device is asked for."""
    yin_track_shapes(x, window, lags, hop, tau_min, threshold)
    return get().yin_track(x, window, lags, hop, tau_min, threshold)


def swd_levels(h, w):
    """gs_swd_levels restated on the host: the number of l >= 0 with min(h, w) >> l >= 16; 0 when there is none, when a size that is halved on
    the way down is odd or when a side exceeds SWD_MAX_SIDE."""
    h, w = int(h), int(w)
    if min(h, w) < 16 or max(h, w) > _lib.SWD_MAX_SIDE:
        return 0
    levels = 0
    while min(h, w) >= 16:
        levels += 1
        if min(h, w) // 2 < 16:
            break
        if (h | w) & 1:
            return 0
        h, w = h // 2, w // 2
    return levels if h >= 7 and w >= 7 else 0


def _swd_tensor(what, name, t, dims, dtypes=(torch.float32,)):
    if not isinstance(t, torch.Tensor) or t.dim() != dims or t.dtype not in dtypes or t.numel() == 0:
        got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
        names = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise ValueError(f"{what}: {name} must be a non-empty {names} tensor of {dims} dimensions (got {got})")


def swd_pyramid_shapes(images):
    """The host side of swd_pyramid: -> (b, h, w, levels) of images [b, 2, h, w] (fp32 or bf16).  ValueError; needs no device."""
    _swd_tensor("swd_pyramid", "images", images, 4, (torch.float32, torch.bfloat16))
    b, c, h, w = (int(s) for s in images.shape)
    if c != 2:
        raise ValueError(f"swd_pyramid: images must have 2 channels (got {c})")
    if b > _lib.SWD_MAX_BATCH:
        raise ValueError(f"swd_pyramid: images must hold at most {_lib.SWD_MAX_BATCH} images a call (got {b})")
    levels = swd_levels(h, w)
    if levels == 0:
        raise ValueError(f"swd_pyramid: images of {h} x {w} have no level (both sides at least 16 and at most {_lib.SWD_MAX_SIDE}, every halved size even)")
    return b, h, w, levels


def swd_pyramid(images):
    """HipKernels.swd_pyramid of the process-wide kernel object; the shape is refused here, before a device is asked for."""
    swd_pyramid_shapes(images)
    return get().swd_pyramid(images)


def swd_patches_shapes(level, ys, xs, desc, row_offset):
    """The host side of swd_patches: -> (b, h, w) of level [b, h, w, 2] (fp32, contiguous); ys, xs contiguous int32 vectors of b * 128; desc a
    contiguous fp32 [rows, 98] matrix that holds rows row_offset .. row_offset + b * 128.  ValueError; needs no device."""
    _swd_tensor("swd_patches", "level", level, 4)
    b, h, w, c = (int(s) for s in level.shape)
    if c != 2 or not level.is_contiguous() or h < 7 or w < 7:
        raise ValueError(f"swd_patches: level must be a contiguous [b, h, w, 2] tensor of at least 7 x 7 (got {tuple(level.shape)})")
    for name, t in (("ys", ys), ("xs", xs)):
        _kmeans_vector("swd_patches", name, t, b * _lib.SWD_PATCHES, torch.int32)
    _swd_tensor("swd_patches", "desc", desc, 2)
    if desc.shape[1] != _lib.SWD_DESC or not desc.is_contiguous() or desc.shape[0] > _lib.SWD_MAX_N:
        raise ValueError(f"swd_patches: desc must be a contiguous [rows, {_lib.SWD_DESC}] matrix of at most {_lib.SWD_MAX_N} rows (got {tuple(desc.shape)})")
    if not 0 <= row_offset <= desc.shape[0] - b * _lib.SWD_PATCHES:
        raise ValueError(f"swd_patches: rows {row_offset} .. {row_offset + b * _lib.SWD_PATCHES} do not lie inside desc of {desc.shape[0]} rows")
    return b, h, w


def swd_desc_shapes(what, desc):
    """desc of swd_moments / swd_project: -> its rows; a contiguous fp32 [rows, 98] matrix of at most SWD_MAX_N rows.  ValueError; needs no device."""
    _swd_tensor(what, "desc", desc, 2)
    if desc.shape[1] != _lib.SWD_DESC or not desc.is_contiguous() or desc.shape[0] > _lib.SWD_MAX_N:
        raise ValueError(f"{what}: desc must be a contiguous [rows, {_lib.SWD_DESC}] matrix of at most {_lib.SWD_MAX_N} rows (got {tuple(desc.shape)})")
    return int(desc.shape[0])


def swd_project_shapes(desc, moments, dirs):
    """The host side of swd_project: -> (n, ndir) of desc [n, 98], moments (float64 [8], swd_moments's result) and dirs [98, ndir] (fp32,
    contiguous, ndir <= SWD_MAX_ROWS).  ValueError; needs no device."""
    n = swd_desc_shapes("swd_project", desc)
    if not isinstance(moments, torch.Tensor) or moments.dtype != torch.float64 or tuple(moments.shape) != (8,) or not moments.is_contiguous():
        raise ValueError("swd_project: moments must be the contiguous float64 vector of 8 that swd_moments returns")
    _swd_tensor("swd_project", "dirs", dirs, 2)
    if dirs.shape[0] != _lib.SWD_DESC or not dirs.is_contiguous() or dirs.shape[1] > _lib.SWD_MAX_ROWS:
        raise ValueError(f"swd_project: dirs must be a contiguous [{_lib.SWD_DESC}, directions] matrix of at most {_lib.SWD_MAX_ROWS} directions (got {tuple(dirs.shape)})")
    return n, int(dirs.shape[1])


def swd_rows_shapes(what, name, t):
    """data of swd_sort, a and b of swd_l1: -> (rows, n) of a contiguous fp32 [rows, n] matrix, rows <= SWD_MAX_ROWS, n <= SWD_MAX_N."""
    _swd_tensor(what, name, t, 2)
    rows, n = int(t.shape[0]), int(t.shape[1])
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous (it is read and written as dense rows)")
    if rows > _lib.SWD_MAX_ROWS or n > _lib.SWD_MAX_N:
        raise ValueError(f"{what}: {name} must have at most {_lib.SWD_MAX_ROWS} rows of at most {_lib.SWD_MAX_N} values (got {rows} x {n})")
    return rows, n


def swd_sort(data):
    """HipKernels.swd_sort of the process-wide kernel object; the shape is refused here, before a device is asked for."""
    swd_rows_shapes("swd_sort", "data", data)
    return get().swd_sort(data)


def swd_l1(a, b):
    """HipKernels.swd_l1 of the process-wide kernel object; the shapes are refused here, before a device is asked for."""
    if swd_rows_shapes("swd_l1", "a", a) != swd_rows_shapes("swd_l1", "b", b):
        raise ValueError(f"swd_l1: a and b differ in shape ({tuple(a.shape)} and {tuple(b.shape)})")
    return get().swd_l1(a, b)


def loudness_shapes(x, rate):
    """The host side of loudness_energy: -> (rows, n) of x ([n] or [rows, n] fp32, rows 1 or 2); rate an integer number of samples per second
    in [LOUDNESS_MIN_RATE, LOUDNESS_MAX_RATE].  ValueError by argument name; needs no device."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2) or x.dtype != torch.float32 or x.numel() == 0:
        got = f"{tuple(x.shape)} {x.dtype}" if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"loudness_energy: x must be a non-empty fp32 vector or [rows, samples] matrix (got {got})")
    rows, n = (1, int(x.shape[0])) if x.dim() == 1 else (int(x.shape[0]), int(x.shape[1]))
    if rows > 2:
        raise ValueError(f"loudness_energy: x must have 1 or 2 rows -- a clip is mono or stereo (got {rows})")
    if not isinstance(rate, (int, np.integer)) or isinstance(rate, bool) or not _lib.LOUDNESS_MIN_RATE <= rate <= _lib.LOUDNESS_MAX_RATE:
        raise ValueError(f"loudness_energy: rate must be an integer number of samples per second in [{_lib.LOUDNESS_MIN_RATE}, "
                         f"{_lib.LOUDNESS_MAX_RATE}] (got {rate!r})")
    return rows, n


def loudness_energy(x, rate):
    """HipKernels.loudness_energy of the process-wide kernel object; the arguments are refused here, before a device is asked for."""
    loudness_shapes(x, rate)
    return get().loudness_energy(x, rate)


def _checked_notes(what, table, rows, length, total, gains):
    """Rows (onset, hold, release, row, *gains) validated and sorted by (onset, position): what both note tables share."""
    fields = ("onset", "hold", "release", "row") + gains
    if len(table) == 0:
        raise ValueError(f"{what}: the table is empty")
    if int(total) <= 0:
        raise ValueError(f"{what}: total must be positive (got {total})")
    checked = []
    for i, entry in enumerate(table):
        if len(entry) != len(fields):
            raise ValueError(f"{what}: note {i} has {len(entry)} fields, not ({', '.join(fields)})")
        onset, hold, release, row = entry[:4]
        for name, v in (("onset", onset), ("hold", hold), ("release", release), ("row", row)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
                raise ValueError(f"{what}: note {i} field '{name}' must be an integer (got {v!r})")
        if not 0 <= onset < total:
            raise ValueError(f"{what}: note {i} field 'onset' = {onset} is outside the clip [0, {total})")
        if not 1 <= hold <= length:
            raise ValueError(f"{what}: note {i} field 'hold' = {hold} is outside [1, {length}]")
        if not 0 <= release <= length - hold:
            raise ValueError(f"{what}: note {i} field 'release' = {release} is outside [0, {length} - hold = {length - hold}]")
        if not 0 <= row < rows:
            raise ValueError(f"{what}: note {i} field 'row' = {row} is outside [0, {rows})")
        for name, gain in zip(gains, entry[4:]):
            if isinstance(gain, bool) or not isinstance(gain, (int, float, np.floating, np.integer)) or not np.isfinite(gain):
                raise ValueError(f"{what}: note {i} field '{name}' must be a finite number (got {gain!r})")
        checked.append((int(onset), int(hold), int(release), int(row)) + tuple(float(g) for g in entry[4:]))
    order = sorted(range(len(checked)), key=lambda i: (checked[i][0], i))
    return [checked[i] for i in order]


class HipKernels(object):
    def __init__(self):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.GansynthHipError("gansynth_amd needs a HIP device (torch.cuda.is_available() is False)")
        _lib.check(self.lib.gs_init(), "gs_init")
        self._param_ranges = []   # (ptr, nbytes) of registered flat parameter buffers
        self._wcache = {}         # (weight ptr, map tag) -> (persistent workspace holding the re-laid operand, stamp)
        self._prep_tables = {}    # tuple of cache keys -> device table of GsPrepDesc rows (refresh_weights)
        self._retired_tables = []  # tables no refresh will use again, kept for the captured graphs that replay them (_weight_ws)
        self._derived = {}        # (parent weight ptr, lo, hi) -> [contiguous slice buffer, stamp, parent, lo, hi] (derived_slice)
        self._folds = None        # deferred bias-gradient folds while deferring: [(partial rows, out, nparts, c)]
        self._pending = None      # deferred weight gradients while deferring: {layer key: {out, bias, [(x, gy, with bias)]}}
        self._guarding = False    # inside stream_guard(): deferred operands are marked with the stream that finally reads them
        self._last_writer = {}    # inside stream_guard(): accumulate target -> (stream, event) of the last call that added into it
        self._early = None        # (min output pixels of a "large" layer, callback): see early_flush_rule
        self._seen = None         # while deferring: {layer key: [pairs recorded so far in this pass, out, bias]}
        self._expected = {}       # pass tag -> {layer key: (pairs of a whole pass, out, bias)}, learned at the final flush of the previous pass
        self._tag = None          # tag of the pass being deferred (defer_wgrad_reductions)
        self._complete = None     # (pred, callback, expected): see complete_rule
        self.ema_steps = 0        # calls of ema_step / ema_step_dev so far (tests: the averaged generator took the HIP path)
        self.ema_steps_dev = 0
        self._resample = {}       # (rate_in, rate_out, device index) -> (GsResample, device table): resample_design
        self._fftconv = {}        # impulse tensor's identity -> (the tensor, its prepared spectrum): fft_convolve_spectrum
        self.fftconv_prepares = 0   # gs_fftconv_prepare calls so far (tests: one per impulse tensor)
        self._loudness = {}       # rate -> GsLoudness: loudness_design
        self._warp_table = {}     # device index -> gs_note_warp's coefficient table there: note_warp_table_dev
        self.note_warps = 0       # gs_note_warp calls so far (tests: a score without a bent note launches none)
        self.loop_searches = self.note_sustains = 0   # gs_loop_search / gs_note_sustain calls so far (tests: no held note, no launch)

    # --------------------------------------------------------- prepared-weight workspaces
    def register_param_buffer(self, flat):
        """Weights living in `flat` may keep their kernel operand (re-laid, storage dtype) between calls."""
        lo, nbytes = flat.data_ptr(), flat.numel() * flat.element_size()
        # A range that overlaps the new buffer belongs to a buffer that no longer exists (an earlier model of this process: the allocator has
        # handed its memory out again).  Left in the list it would be the FIRST match of a weight of the new buffer that lies inside it, while
        # invalidate_weights(flat) only reaches the ranges that hold the new buffer's first byte: after an optimizer step that weight's
        # operand would pass for fresh and the layer would run one update behind its parameters.  The dead range goes, with the operands
        # and slices that hang on it (kept alive, like the retired tables, for a captured graph that may still replay them).
        dead = [r for r in self._param_ranges if r[0] < lo + nbytes and lo < r[0] + r[1]]
        if dead:
            self._param_ranges = [r for r in self._param_ranges if not any(r is d for d in dead)]
            for key in [k for k, e in self._wcache.items() if any(e[4] is d for d in dead)]:
                self._retired_tables.append(self._wcache.pop(key))
            for key in [k for k in self._derived if lo <= k[0] < lo + nbytes]:
                self._retired_tables.append(self._derived.pop(key))
            self._retired_tables.extend(self._prep_tables.values())
            self._prep_tables.clear()
        self._param_ranges.append([lo, nbytes, 0])

    def invalidate_weights(self, flat=None):
        """Parameter values changed (all registered buffers, or only the one `flat` lives in)."""
        ptr = None if flat is None else flat.data_ptr()
        for rng in self._param_ranges:
            if ptr is None or rng[0] <= ptr < rng[0] + rng[1]:
                rng[2] += 1

    def _weight_ws(self, w, tag, nbytes, plan=None):
        """-> (workspace, w_prepared).  A registered parameter gets one persistent workspace per conv map, reused
        (w_prepared = 1) until the parameter values change; anything else gets a transient workspace.
        `plan` = (GS_PREP_* map, ci, co, ksize, stride, dtype id) lets refresh_weights() rebuild the operand in a batch."""
        ptr = w.data_ptr()
        rng = next((r for r in self._param_ranges if r[0] <= ptr < r[0] + r[1]), None)
        if rng is None:
            return _ws(nbytes, w.device), 0
        key, stamp = (ptr, tag), (rng[2], w._version)
        ent = self._wcache.get(key)
        if ent is not None and ent[0].numel() >= nbytes:
            if ent[1] == stamp:
                return ent[0], 1
            ent[1] = stamp
            return ent[0], 0
        self._wcache[key] = [_ws(nbytes, w.device), stamp, w, plan, rng]
        # (a new workspace changes the rows: the tables are built again by the next refresh.  The old ones stay ALIVE: a captured graph
        #  replays gs_weight_prep_batch on a table's address, and a second model built in the same process -- new weights, new keys -- must
        #  not hand that memory back to the allocator under the first one's graph.  A few KB each.)
        self._retired_tables.extend(self._prep_tables.values())
        self._prep_tables.clear()
        return self._wcache[key][0], 0

    def _stamp(self, w):
        ptr = w.data_ptr()
        rng = next((r for r in self._param_ranges if r[0] <= ptr < r[0] + r[1]), None)
        return (None if rng is None else rng[2], w._version)

    def derived_slice(self, w, lo, hi):
        """A persistent contiguous copy of w[:, :, lo:hi, :] (the 257-input-channel conv of the last discriminator block runs as
        two convs on slices of ONE variable): refreshed when the parent changes -- here on use, and by refresh_weights() right
        after an optimizer step -- so that a pass neither copies the slice nor re-lays its kernel operands every time, and a
        captured graph contains neither.  Returns an alias (fresh tensor object, same storage)."""
        key = (w.data_ptr(), int(lo), int(hi))
        ent = self._derived.get(key)
        stamp = self._stamp(w)
        with torch.no_grad():
            if ent is None or ent[0].shape[2] != hi - lo or ent[0].shape != w[:, :, lo:hi, :].shape:
                buf = w.detach()[:, :, lo:hi, :].contiguous()
                self.register_param_buffer(buf)
                ent = self._derived[key] = [buf, stamp, w, int(lo), int(hi)]
            elif ent[1] != stamp:
                self._refresh_derived(ent, w)
        return ent[0].detach()

    def _refresh_derived(self, ent, w):
        ent[0].copy_(w.detach()[:, :, ent[3]:ent[4], :])
        ent[1], ent[2] = self._stamp(w), w
        self.invalidate_weights(ent[0])

    def refresh_weights(self, flat=None):
        """Rebuild, in ONE launch, every stale prepared operand of the parameters living in `flat` (all registered
        buffers when None) -- called after an optimizer step instead of letting each conv re-lay its weight."""
        extra = []   # registered ranges of the derived slices refreshed here: their operands join the ONE launch below
        if self._derived:   # slices of parameters first (a copy each), then their operands together with everything else
            lo_, hi_ = (None, None) if flat is None else (flat.data_ptr(), flat.data_ptr() + flat.numel() * flat.element_size())
            with torch.no_grad():
                for ent in self._derived.values():
                    w = ent[2]
                    if (lo_ is None or lo_ <= w.data_ptr() < hi_) and ent[1] != self._stamp(w):
                        self._refresh_derived(ent, w)
                        extra.append(ent[0].data_ptr())
        ptr = None if flat is None else flat.data_ptr()

        def wanted(rng):
            return ptr is None or rng[0] <= ptr < rng[0] + rng[1] or any(rng[0] <= q < rng[0] + rng[1] for q in extra)

        stale = [k for k, e in self._wcache.items() if e[3] is not None and wanted(e[4]) and e[1] != (e[4][2], e[2]._version)]
        if not stale:
            return 0
        tkey = tuple(stale)
        table = self._prep_tables.get(tkey)
        if table is None:
            rows = np.zeros((len(stale), 5), dtype=np.int64)   # GsPrepDesc: 2 pointers + 6 int32 = 40 bytes
            for i, k in enumerate(stale):
                buf, _, w, plan, _ = self._wcache[k]
                rows[i, 0], rows[i, 1] = w.data_ptr(), buf.data_ptr()
                rows[i, 2:5] = np.array(plan, dtype=np.int32).view(np.int64)
            table = torch.from_numpy(rows).to(self._wcache[stale[0]][0].device)
            self._prep_tables[tkey] = table
        _lib.check(self.lib.gs_weight_prep_batch(table.data_ptr(), len(stale), _stream()), "gs_weight_prep_batch")
        for k in stale:
            e = self._wcache[k]
            e[1] = (e[4][2], e[2]._version)
        return len(stale)

    # ------------------------------------------------- accumulate targets on more than one stream
    @contextlib.contextmanager
    def _adds_into(self, *targets):
        """Around a launch that ADDS into `targets` (a variable's gradient) right away.  Inside stream_guard() two passes on two streams may
        add into the same variable -- the real and the fake pass of a discriminator run: the launch waits for the last one that touched the
        target from the other stream and leaves its own event behind (the host's issue order, which is also the order the one-stream
        schedule uses).  Calls that only RECORD a deferred job, or leave partial rows for the batched fold, do not come through here: the
        R1 double-backward's first recorded layer must not wait for the end of the fake pass's backward."""
        if not self._guarding:
            yield
            return
        stream = torch.cuda.current_stream()
        targets = [t for t in targets if isinstance(t, torch.Tensor) and t.is_cuda]
        spans = [self._span(t) for t in targets]
        for lo, hi in spans:
            # (by ADDRESS RANGE, not by pointer: a channel slice w.grad[:, :, lo:hi, :] of a wider variable -- wgrad_slice_target_ok -- and its
            #  parent, or two slices, are the same memory under different pointers)
            for (plo, phi), (pstream, pev) in self._last_writer.items():
                if plo < hi and lo < phi and pstream != stream.cuda_stream:
                    stream.wait_event(pev)
        yield
        for span in spans:
            ev = torch.cuda.Event()
            ev.record(stream)
            for old in [k for k in self._last_writer if k[0] < span[1] and span[0] < k[1] and k != span]:
                # an overlapping older entry stays only where it reaches beyond the new one (its event still orders that part)
                if span[0] <= old[0] and old[1] <= span[1]:
                    del self._last_writer[old]
            self._last_writer[span] = (stream.cuda_stream, ev)

    @staticmethod
    def _span(t):
        """[first byte, one past the last byte) a (possibly strided) tensor touches."""
        lo = t.data_ptr()
        return lo, lo + (sum((n - 1) * st for n, st in zip(t.shape, t.stride()) if n > 0) + 1) * t.element_size()

    # ----------------------------------------------------------- deferred weight gradients
    def defer_wgrad_reductions(self, tag=None):
        """`tag`: names the KIND of pass (the trainer's "d" / "g") -- the pairs each layer receives in a pass are remembered per tag (complete_rule).
        From now on the in-place (`out=`) conv weight gradients are only RECORDED; flush_wgrad_reductions() then runs, per
        weight, ONE multi-source launch over all recorded (x, gy) pairs of that layer (real + fake discriminator pass, the
        second-order contribution of the penalty terms ...) and folds the slice partials of all layers in a handful of launches.
        A backward pass has ~70 such gradients, each otherwise its own partials + reduction.  The `out` buffers are complete
        only after the flush; x and gy are kept alive (and must not be written) until then."""
        if self._pending is None:
            self._pending = {}
            self._folds = None if config.value("GS_NO_DEFERRED_FOLDS") else []
            self._seen, self._tag, self._complete = {}, tag, None

    def _partial_rows(self, producer, p, c, dt, out):
        """While gradients are deferred: a buffer of its own for the partial rows of a bias gradient that is ADDED into `out` (a
        variable's .grad, only read after the flush) -- the producer then skips its fold and flush_wgrad_reductions() folds all
        of them in one launch (gs_channel_fold_batch).  None: fold right away."""
        if self._folds is None or out is None:
            return None
        rows = self.lib.gs_bias_partial_rows(producer, p, c, dt)
        if rows <= 0:
            return None
        part = torch.empty((rows * c,), dtype=torch.float32, device=out.device)
        self._folds.append((part, out, rows, c))
        return part

    def _flush_folds(self):
        folds, self._folds = self._folds, None
        if not folds:
            return
        if self._guarding:   # (a partial written on a forked branch is read here, on the flushing stream)
            _StreamGuard._mark([f[0] for f in folds], torch.cuda.current_stream())
        arr = (_lib.GsFoldJob * len(folds))()
        for jb, (part, out, rows, c) in zip(arr, folds):
            jb.part, jb.out, jb.nparts, jb.c, jb.accumulate = part.data_ptr(), out.data_ptr(), rows, c, 1
        ptr = ctypes.cast(arr, ctypes.c_void_p)
        ws = _ws(max(self.lib.gs_channel_fold_batch_workspace_bytes(ptr, len(folds)), 256), folds[0][1].device)
        _lib.check(self.lib.gs_channel_fold_batch(ptr, len(folds), ws.data_ptr(), ws.numel(), _stream()), "gs_channel_fold_batch")

    def wgrad_slice_target_ok(self, x, co, ksize, stride):
        """May a conv weight gradient be added into a CHANNEL SLICE w.grad[:, :, lo:hi, :] of a wider variable (a strided `out`)?
        Only while gradients are deferred, for the layers gs_conv_wgrad_jobs runs grouped (bf16, 3x3, >= 64 channels both sides) and
        for the 1-input-channel plane conv of the direct kernel."""
        if self._pending is None or config.value("GS_NO_WGRAD_GROUPS") or ksize != 3:
            return False
        if x.shape[1] == 1 and stride == 1 and co % 4 == 0:   # the 1-channel direct kernel: its slice reduction stays pending, the batched fold takes the stride
            return True
        return x.dtype == torch.bfloat16 and x.shape[1] % 64 == 0 and co % 64 == 0

    # Large layers first.  A backward pass walks the pyramid top-down (and the second-order passes walk it bottom-up first): by the time it
    # reaches the few-block levels every (x, gy) pair of the full-chip levels recorded so far is final, and their contraction -- the
    # HBM-bound part of the weight gradients -- needs nothing the chain below still computes.  Rule: when a SMALL layer is recorded while
    # LARGE ones are pending, `callback(select)` is called once; the trainer answers with flush_wgrad_reductions(select=select) on a forked
    # branch of the run's hipGraph (models.GANSynth._early_flush), where it runs beside the latency-bound chain instead of after it.  A layer
    # whose pairs arrive on both sides of that point (the discriminator's: the R1 pairs early, the real / fake pairs late) is contracted in
    # two launches that add into the same gradient; the rule depends on the recorded sequence only, never on the stream.
    # Complete layers early.  The pairs a layer receives in a pass of a given kind are the same every time (the real pass, the fake pass, the
    # second-order terms): once every layer `pred` picks has received as many as in the previous pass of that kind, their gradients need nothing
    # the backward still computes -- `callback(select, others)` is called once, from inside the node that recorded the last pair, and the trainer
    # answers with flush_wgrad_reductions(select=select) and whatever wants COMPLETE gradients early (data parallel: their all-reduce, beside
    # the rest of the backward).  `others`: [(out, bias)] of every layer of the pass `pred` does not pick -- what is NOT complete then.
    def complete_rule(self, pred, callback):
        exp = self._expected.get(self._tag) if self._tag is not None else None
        self._complete = (pred, callback, exp) if (callback is not None and exp and any(pred(k) for k in exp)) else None
        return self._complete is not None

    def flush_bias_folds(self):
        """The bias-gradient folds recorded so far, now (the rest stay deferred to the final flush)."""
        if self._pending is not None and self._folds:
            self._flush_folds()
            self._folds = []

    def early_flush_rule(self, min_pixels, callback):
        """`min_pixels`: one threshold or several (descending): each fires once per arming, for the layers at or above it."""
        if callback is None:
            self._early = None
            return
        ts = sorted({int(t) for t in (min_pixels if isinstance(min_pixels, (tuple, list)) else (min_pixels,))}, reverse=True)
        self._early = (ts, callback, set())

    @staticmethod
    def _key_pixels(key):
        return int(key[6][1]) * int(key[6][2])   # (output positions of the conv whose weight this is)

    def _defer_wgrad(self, key, x, gy, out, bias_out):
        if self._early is not None and self._pending:
            px = self._key_pixels(key)
            for big in self._early[0]:
                if px < big and big not in self._early[2] and any(self._key_pixels(k) >= big for k in self._pending):
                    self._early[2].add(big)
                    self._early[1](lambda k, big=big: self._key_pixels(k) >= big)
        grp = self._pending.setdefault(key, {"out": out, "bias": None, "src": []})
        if bias_out is not None:
            assert grp["bias"] is None or grp["bias"].data_ptr() == bias_out.data_ptr()
            grp["bias"] = bias_out
        grp["src"].append((x, gy, bias_out is not None))
        if self._seen is not None:
            rec = self._seen.setdefault(key, [0, out, bias_out])
            rec[0] += 1
            if bias_out is not None:
                rec[2] = bias_out
            if self._complete is not None and self._complete[0](key):
                pred, callback, exp = self._complete
                if all(self._seen.get(k, (0,))[0] >= e[0] for k, e in exp.items() if pred(k)):
                    self._complete = None
                    callback(pred, [(e[1], e[2]) for k, e in exp.items() if not pred(k)])

    def flush_wgrad_reductions(self, group_of=None, on_group_done=None, select=None, split_stream=None, on_rest_done=None):
        """`group_of(out.data_ptr()) -> int | None` orders the layers into groups (the trainer's gradient buckets, in completion
        order); each group is contracted and folded before the next one starts and `on_group_done(group)` is called right after
        its last launch -- the data-parallel trainer puts that bucket's all-reduce on the wire there."""
        if select is not None:   # (the recorded layers `select(key)` picks, now; everything else -- and the bias folds -- stays pending)
            picked = {k: self._pending.pop(k) for k in [k for k in self._pending if select(k)]}
            return self._flush_groups(picked) if picked else 0
        groups, self._pending = self._pending, None
        if self._seen is not None and self._tag is not None:
            self._expected[self._tag] = {k: (v[0], v[1], v[2]) for k, v in self._seen.items()}
        self._seen, self._complete = None, None
        self._flush_folds()   # (bias gradients first: they belong to the same buckets as the weights folded below)
        if not groups:
            return 0
        if group_of is not None:
            tagged = {}
            for key, grp in groups.items():
                # a deferred layer writes its weight gradient AND (through the same launches) its bias gradient: it runs with the
                # EARLIER of their two buckets, or that one would go on the wire before the job has added into it
                tagged.setdefault(completion_group(group_of, grp["out"], grp["bias"]), []).append((key, grp))
            order = sorted((g for g in tagged if g is not None)) + ([None] if None in tagged else [])
            n = 0
            for g in order:
                n += self._flush_groups(dict(tagged[g]))
                if g is not None and on_group_done is not None:
                    on_group_done(g)
            return n
        return self._flush_groups(groups, split_stream, on_rest_done)

    def _flush_groups(self, groups, split_stream=None, on_rest_done=None):
        """One gs_conv_wgrad_jobs call for every recorded layer of `groups`: the library groups the layers by kernel
        instantiation (one stream-K launch + one fold per group) and batches the rest.
        `split_stream` (a captured run's idle branch stream): the HBM-bound jobs -- the <= 32-input-channel layers at the top of the pyramid,
        streaming kernels -- go THERE, beside the MFMA-bound grouped contractions of the other layers on this stream: the jobs of a flush are
        independent of each other, one launch after the other on one stream each of them has the chip to itself with half of it idle."""
        if split_stream is not None and self._guarding and len(groups) > 1:
            thin = {k: g for k, g in groups.items() if int(k[5][0]) <= 32}
            rest = {k: g for k, g in groups.items() if int(k[5][0]) > 32}
            if thin and rest and on_rest_done is not None:
                # data parallel: the grouped contractions FIRST -- they complete every gradient in front of the thin layers' in the flat buffer,
                # i.e. nearly all of its bytes -- then `on_rest_done(thin)` puts that part on the wire on this stream while the thin layers are
                # contracted beside it on the branch (which starts behind the grouped launches, not beside them: the collective takes their place)
                main = torch.cuda.current_stream()
                n = self._flush_groups(rest)
                split_stream.wait_stream(main)
                on_rest_done(thin)
                with torch.cuda.stream(split_stream):
                    n += self._flush_groups(thin)
                main.wait_stream(split_stream)
                return n
            if thin and rest:
                # (a THIRD stream for the stride-2 / transposed layers' grouped launch beside the stride-1 layers': measured neutral, 5.01 / 5.01 ms)
                main = torch.cuda.current_stream()
                split_stream.wait_stream(main)
                with torch.cuda.stream(split_stream):
                    n = self._flush_groups(thin)
                n += self._flush_groups(rest)
                main.wait_stream(split_stream)
                return n
        jobs, keep = [], []
        for key, grp in groups.items():
            kind, ksize, stride, alpha = key[0], key[2], key[3], key[4]
            out, bias, src = grp["out"], grp["bias"], grp["src"]
            if self._guarding:   # (recorded on whatever stream the backward node ran on, read on the flushing stream)
                _StreamGuard._mark([(x, gy) for x, gy, _ in src], torch.cuda.current_stream())
            _, ci, h, wd = src[0][0].shape   # (the pairs of a layer may differ in their image counts)
            co = src[0][1].shape[1]
            dt = _dt(src[0][0])
            for i in range(0, len(src), _lib.WGRAD_MAX_SOURCES):
                part = src[i:i + _lib.WGRAD_MAX_SOURCES]
                jb = _lib.GsWgradJob()
                for s_, (x, gy, wb) in enumerate(part):
                    jb.x[s_], jb.gy[s_], jb.n[s_] = x.data_ptr(), gy.data_ptr(), x.shape[0]
                jb.nsrc = len(part)
                jb.bias_mask = sum(1 << j for j, p in enumerate(part) if p[2]) if kind == "conv" else 0
                jb.gw = out.data_ptr()
                jb.gb = bias.data_ptr() if (kind == "conv" and bias is not None and jb.bias_mask) else None
                jb.h, jb.w, jb.ci, jb.co, jb.ksize, jb.stride = h, wd, ci, co, ksize, stride
                jb.transposed = 0 if kind == "conv" else 1
                jb.alpha, jb.accumulate, jb.dtype = float(alpha), 1, dt
                if not out.is_contiguous():   # [:, :, lo:hi, :] of a wider variable's gradient (wgrad_slice_target_ok)
                    assert kind == "conv" and out.stride(3) == 1 and out.stride(2) == co and out.stride(1) % co == 0 and out.stride(0) == ksize * out.stride(1)
                    jb.gw_ci_stride = out.stride(1) // co
                jobs.append(jb)
                keep.append(part)
        if jobs:
            arr = (_lib.GsWgradJob * len(jobs))(*jobs)
            ptr = ctypes.cast(arr, ctypes.c_void_p)
            nb = self.lib.gs_conv_wgrad_jobs_workspace_bytes(ptr, len(jobs))
            ws = _ws(nb, groups[next(iter(groups))]["out"].device)
            _lib.check(self.lib.gs_conv_wgrad_jobs(ptr, len(jobs), ws.data_ptr(), ws.numel(), _stream()), "gs_conv_wgrad_jobs")
        return sum(len(g["src"]) for g in groups.values())   # (workspaces and sources die here: later launches are stream-ordered behind)

    # ------------------------------------------------------------------------------- conv
    def _conv(self, which, w, alpha, dt, n, ci, h, wd, co, ksize=3, stride=2, transposed=False, device=None):
        """-> (GsConv of the layer with its workspace for map `which` attached, that workspace).  (n, ci, h, wd): the layer's forward input.
        A forward / data-gradient map keeps its re-laid weight in a persistent workspace per (weight, map) (_weight_ws); a weight gradient
        (w None) gets a transient one on `device`."""
        c = _lib.GsConv(n, h, wd, ci, co, ksize, stride, 1 if transposed else 0, dt, 0, float(alpha), None, 0)
        nb = self.lib.gs_conv_workspace_bytes(c, which)
        if which == _lib.CONV_BWD_WEIGHT:
            ws = _ws(nb, device)
        elif transposed:
            tag, prep = (("t_fwd", _lib.PREP_CONVT_FWD) if which == _lib.CONV_FWD else ("t_bwd_data", _lib.PREP_CONVT_BWD_DATA))
            ws, c.w_prepared = self._weight_ws(w, (tag, dt), nb, (prep, ci, co, 3, 2, dt))
        else:
            tag, prep = (("fwd", _lib.PREP_CONV_FWD) if which == _lib.CONV_FWD else ("bwd_data", _lib.PREP_CONV_BWD_DATA))
            ws, c.w_prepared = self._weight_ws(w, (tag, ksize, stride, dt), nb, (prep, ci, co, ksize, stride, dt))
        c.ws, c.ws_bytes = ws.data_ptr(), ws.numel()
        return c, ws

    def _conv_fwd(self, x, w, bias, act, ksize, stride, transposed, alpha, y, y_norm=None, eps=0.0):
        """The forward map of either conv kind into the outputs the caller allocated (x, w kernel-ready)."""
        n, ci, h, wd = x.shape
        c, ws = self._conv(_lib.CONV_FWD, w, alpha, _dt(x), n, ci, h, wd, w.shape[3], ksize, stride, transposed)
        bp = None if bias is None else _f32c(bias).data_ptr()
        _lib.check(self.lib.gs_conv_fwd(c, x.data_ptr(), w.data_ptr(), bp, int(act), None if y is None else y.data_ptr(),
                                        None if y_norm is None else y_norm.data_ptr(), float(eps), _stream()), "gs_conv_fwd")

    @staticmethod
    def _out_shape(x, co, stride, transposed):
        n, _, h, wd = x.shape
        return (n, co, 2 * h, 2 * wd) if transposed else (n, co, h // stride, wd // stride)

    def conv2d_fwd(self, x, w, ksize, stride, alpha):
        return self.conv2d_fwd_bias_act(x, w, None, ksize, stride, alpha, _lib.ACT_NONE)

    def conv2d_fwd_mask(self, x, w, ksize, stride, alpha, mask, mask_act):
        """conv2d_fwd(x, w) * mask_act'(.) through `mask` (an activation output of the result's shape) in one pass."""
        x, w, mask = _act(x), _f32c(w), _act(mask)
        n, ci, h, wd = x.shape
        y = _empty_like_act(self._out_shape(x, w.shape[3], stride, False), x)
        assert mask.shape == y.shape and mask.dtype == y.dtype
        c, ws = self._conv(_lib.CONV_FWD, w, alpha, _dt(x), n, ci, h, wd, w.shape[3], ksize, stride)
        _lib.check(self.lib.gs_conv_fwd_mask(c, x.data_ptr(), w.data_ptr(), mask.data_ptr(), _mask_act(mask, mask_act), y.data_ptr(), _stream()), "gs_conv_fwd_mask")
        return y

    def conv2d_fwd_bias_act(self, x, w, bias, ksize, stride, alpha, act, bits=None):
        """`bits` (default: whenever the result qualifies, 1/16 more bytes written): the leaky-relu result carries its sign bits behind it."""
        x, w = _act(x), _f32c(w)
        co = w.shape[3]
        bits = _bits_wanted(x, co, act) and bits is not False
        y = (_empty_act_with_bits if bits else _empty_like_act)(self._out_shape(x, co, stride, False), x)
        self._conv_fwd(x, w, bias, act | (_lib.ACT_WRITE_BITS if bits else 0), ksize, stride, False, alpha, y)
        return y

    def conv2d_fwd_bias_act_norm(self, x, w, bias, ksize, stride, alpha, act, eps, want_z=True):
        """(z, y): z = act(alpha * conv + bias), y = pixel_norm(z) -- one launch where the conv tile owns all channels of a pixel;
        z is None with want_z=False (no backward will need the activation)."""
        return self._fwd_bias_act_norm(x, w, bias, ksize, stride, False, alpha, act, eps, want_z)

    def _fwd_bias_act_norm(self, x, w, bias, ksize, stride, transposed, alpha, act, eps, want_z):
        x, w = _act(x), _f32c(w)
        shape = self._out_shape(x, w.shape[3], stride, transposed)
        y = _empty_like_act(shape, x)
        z = _empty_like_act(shape, x) if want_z else None
        self._conv_fwd(x, w, bias, act, ksize, stride, transposed, alpha, z, y, eps)
        return z, y

    def conv2d_transpose_fwd_bias_act_norm(self, x, w, bias, alpha, act, eps, want_z=True):
        return self._fwd_bias_act_norm(x, w, bias, 3, 2, True, alpha, act, eps, want_z)

    def conv2d_bwd_data(self, gy, w, x_shape, ksize, stride, alpha, mask=None, mask_act=0):
        """gx, or with `mask` (the conv's forward input, itself the output of activation `mask_act`) gx * act'(.): the data
        gradient w.r.t. the previous layer's pre-activation in one pass."""
        return self._bwd_data(gy, w, x_shape, ksize, stride, False, alpha, mask, mask_act)

    def _bwd_data(self, gy, w, x_shape, ksize, stride, transposed, alpha, mask=None, mask_act=0):
        gy, w = _act(gy), _f32c(w)
        n, ci, h, wd = x_shape
        gx = _empty_like_act((n, ci, h, wd), gy)
        c, ws = self._conv(_lib.CONV_BWD_DATA, w, alpha, _dt(gy), n, ci, h, wd, w.shape[3], ksize, stride, transposed)
        mp = None
        if mask is not None:
            mask = _act(mask)
            assert mask.shape == gx.shape and mask.dtype == gx.dtype
            mp = mask.data_ptr()
        _lib.check(self.lib.gs_conv_bwd_data(c, gy.data_ptr(), w.data_ptr(), mp, _mask_act(mask, mask_act) if mask is not None else 0, gx.data_ptr(), _stream()),
                   "gs_conv_bwd_data")
        return gx

    def _is_fused(self, query, x_shape, co, ksize, stride, transposed, dtype):
        n, ci, h, wd = (int(v) for v in x_shape)
        dt = GS_F32 if dtype == torch.float32 else GS_BF16
        return bool(query(_lib.GsConv(n, h, wd, ci, int(co), int(ksize), int(stride), 1 if transposed else 0, dt)))

    def fwd_pnbwdbwd_is_fused(self, x_shape, co, ksize, stride, transposed, dtype):
        """Does conv2d[_transpose]_fwd_pnbwdbwd run as ONE launch for a conv with input x_shape and `co` output channels?"""
        return self._is_fused(self.lib.gs_conv_fwd_pnbwdbwd_is_fused, x_shape, co, ksize, stride, transposed, dtype)

    def conv2d_fwd_pnbwdbwd(self, x, w, ksize, stride, alpha, g, z, eps, act):
        """(out_z, out_g) = both gradients of u = act'(z) pixel_norm_bwd(g, z) contracted with t = conv2d_fwd(x, w): what pixel_norm_bwd_bwd(t, g, z,
        pre_act=act, with_g=True) returns, from the conv's epilogue where its tile owns all channels of a pixel."""
        return self._fwd_pnbwdbwd(x, w, ksize, stride, False, alpha, g, z, eps, act)

    def _fwd_pnbwdbwd(self, x, w, ksize, stride, transposed, alpha, g, z, eps, act):
        x, w, g, z = _act(x), _f32c(w), _act(g), _act(z)
        n, ci, h, wd = x.shape
        out_g = _empty_like_act(self._out_shape(x, w.shape[3], stride, transposed), x)
        assert g.shape == out_g.shape == z.shape and g.dtype == x.dtype == z.dtype
        out_z = torch.empty_like(out_g)
        c, ws = self._conv(_lib.CONV_FWD, w, alpha, _dt(x), n, ci, h, wd, w.shape[3], ksize, stride, transposed)
        _lib.check(self.lib.gs_conv_fwd_pnbwdbwd(c, x.data_ptr(), w.data_ptr(), g.data_ptr(), z.data_ptr(), int(act), float(eps), out_g.data_ptr(), out_z.data_ptr(),
                                                 _stream()), "gs_conv_fwd_pnbwdbwd")
        return out_z, out_g

    def conv2d_transpose_fwd_pnbwdbwd(self, x, w, alpha, g, z, eps, act):
        return self._fwd_pnbwdbwd(x, w, 3, 2, True, alpha, g, z, eps, act)

    def bwd_data_pnbwd_is_fused(self, x_shape, co, ksize, stride, transposed, dtype):
        """Does conv2d[_transpose]_bwd_data_pnbwd run as ONE launch for a conv with input x_shape = (n, ci, h, w) and `co` output channels?"""
        return self._is_fused(self.lib.gs_conv_bwd_data_pnbwd_is_fused, x_shape, co, ksize, stride, transposed, dtype)

    def conv2d_bwd_data_pnbwd(self, gy, w, x_shape, ksize, stride, alpha, z, eps, act, addend=None):
        """(pixel_norm_bwd(conv2d_bwd_data(gy, w), z) + addend) * act'(z): the data gradient continued through the previous block's pixel norm
        and activation (z: that block's activation output, x_shape's shape) -- one launch where the conv tile owns all channels of a pixel."""
        return self._bwd_data_pnbwd(gy, w, x_shape, ksize, stride, False, alpha, z, eps, act, addend)

    def _bwd_data_pnbwd(self, gy, w, x_shape, ksize, stride, transposed, alpha, z, eps, act, addend):
        gy, w, z = _act(gy), _f32c(w), _act(z)
        n, ci, h, wd = x_shape
        assert tuple(z.shape) == (n, ci, h, wd) and z.dtype == gy.dtype
        gx = _empty_like_act((n, ci, h, wd), gy)
        c, ws = self._conv(_lib.CONV_BWD_DATA, w, alpha, _dt(gy), n, ci, h, wd, w.shape[3], ksize, stride, transposed)
        ap = None
        if addend is not None:
            addend = _match(addend, z)
            ap = addend.data_ptr()
        _lib.check(self.lib.gs_conv_bwd_data_pnbwd(c, gy.data_ptr(), w.data_ptr(), z.data_ptr(), ap, int(act), float(eps), gx.data_ptr(), _stream()),
                   "gs_conv_bwd_data_pnbwd")
        return gx

    def conv2d_transpose_bwd_data_pnbwd(self, gy, w, alpha, z, eps, act, addend=None):
        """The same behind a transposed conv (its data gradient is the stride-2 conv)."""
        n, _, h2, w2 = gy.shape
        return self._bwd_data_pnbwd(gy, w, (n, w.shape[2], h2 // 2, w2 // 2), 3, 2, True, alpha, z, eps, act, addend)

    def conv2d_bwd_weight(self, x, gy, ksize, stride, alpha, out=None, bias_out=None):
        """gw (new tensor), or with `out` (fp32, contiguous) the gradient is ADDED into it inside the kernel.  With `bias_out`
        (needs `out`) the bias gradient sum_{n,h,w} gy is added into it by the same launches."""
        return self._bwd_weight(x, gy, ksize, stride, False, alpha, out, bias_out)

    def _bwd_weight(self, x, gy, ksize, stride, transposed, alpha, out, bias_out):
        x, gy = _act(x), _act(gy)
        n, ci, h, wd = x.shape
        co = gy.shape[1]
        gw = torch.empty((ksize, ksize, ci, co), dtype=torch.float32, device=x.device) if out is None else out
        if bias_out is not None:
            assert out is not None and bias_out.dtype == torch.float32 and bias_out.is_contiguous()
        if out is not None and self._pending is not None:
            self._defer_wgrad(("convT" if transposed else "conv", out.data_ptr(), ksize, stride, float(alpha), tuple(x.shape[1:]), tuple(gy.shape[1:]), x.dtype),
                              x, gy, out, bias_out)
            return gw
        assert out is None or transposed or out.is_contiguous(), "a channel-slice target needs deferred gradients (wgrad_slice_target_ok)"
        c, ws = self._conv(_lib.CONV_BWD_WEIGHT, None, alpha, _dt(x), n, ci, h, wd, co, ksize, stride, transposed, device=x.device)
        with self._adds_into(out, bias_out):
            _lib.check(self.lib.gs_conv_bwd_weight(c, x.data_ptr(), gy.data_ptr(), gw.data_ptr(), None if bias_out is None else bias_out.data_ptr(),
                                                   0 if out is None else 1, _stream()), "gs_conv_bwd_weight")
        return gw

    def conv2d_transpose_fwd(self, x, w, alpha):
        return self.conv2d_transpose_fwd_bias_act(x, w, None, alpha, _lib.ACT_NONE)

    def conv2d_transpose_fwd_bias_act(self, x, w, bias, alpha, act):
        x, w = _act(x), _f32c(w)
        y = _empty_like_act(self._out_shape(x, w.shape[3], 2, True), x)
        self._conv_fwd(x, w, bias, act, 3, 2, True, alpha, y)
        return y

    def conv2d_transpose_bwd_data(self, gy, w, alpha):
        n, _, h2, w2 = gy.shape
        return self._bwd_data(gy, w, (n, w.shape[2], h2 // 2, w2 // 2), 3, 2, True, alpha)

    def conv2d_transpose_bwd_weight(self, x, gy, alpha, out=None):
        return self._bwd_weight(x, gy, 3, 2, True, alpha, out, None)

    # ------------------------------------------------------------------------------ dense
    # x is [b, in], or the channels-last [n, c, h, w] activation whose tf.layers.flatten (NCHW) feeds the layer (networks.py:185-186): w stays
    # [c * h * w, out] in the reference's row order, the flatten is a row map inside the kernels
    @staticmethod
    def _dense(x, out, alpha, like):
        """The GsDense of a layer from its input side (a tensor or its shape), its width and a tensor of the activations' dtype."""
        shape = tuple(x.shape) if isinstance(x, torch.Tensor) else tuple(x)
        c, hw = (shape[1], shape[2] * shape[3]) if len(shape) == 4 else (0, 0)
        return _lib.GsDense(shape[0], c * hw if c else shape[1], out, c, hw, _dt(like), float(alpha), None, 0)

    def _dense_fwd(self, x, w, bias, alpha, act):
        x, w = _act(x), _f32c(w)
        d = self._dense(x, w.shape[1], alpha, x)
        y = torch.empty((d.b, d.out), dtype=x.dtype, device=x.device)
        ws = _ws(self.lib.gs_dense_fwd_workspace_bytes(d), x.device)
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
        _lib.check(self.lib.gs_dense_fwd(d, x.data_ptr(), w.data_ptr(), None if bias is None else _f32c(bias).data_ptr(), int(act), y.data_ptr(), _stream()), "gs_dense_fwd")
        return y

    def _dense_bwd_data(self, gy, w, x_shape, alpha):
        gy, w = _act(gy), _f32c(w)
        d = self._dense(x_shape, gy.shape[1], alpha, gy)
        gx = torch.empty(tuple(x_shape), dtype=gy.dtype, device=gy.device, memory_format=CL if len(x_shape) == 4 else torch.contiguous_format)
        _lib.check(self.lib.gs_dense_bwd_data(d, gy.data_ptr(), w.data_ptr(), gx.data_ptr(), _stream()), "gs_dense_bwd_data")
        return gx

    # (dense weight gradients deferred to the final contraction like the convs' -- off the backward's chain, beside the MFMA-bound jobs: measured
    #  neutral, 5.083 -> 5.09 ms, round 6; they are launched where autograd produces them)
    def _dense_bwd_weight(self, x, gy, alpha, out):
        x, gy = _act(x), _act(gy)
        d = self._dense(x, gy.shape[1], alpha, x)
        gw = torch.empty((d.inp, d.out), dtype=torch.float32, device=x.device) if out is None else out
        with self._adds_into(out):
            _lib.check(self.lib.gs_dense_bwd_weight(d, x.data_ptr(), gy.data_ptr(), gw.data_ptr(), 0 if out is None else 1, _stream()), "gs_dense_bwd_weight")
        return gw

    def dense_fwd(self, x, w, alpha):
        return self._dense_fwd(x, w, None, alpha, _lib.ACT_NONE)

    def dense_fwd_bias_act(self, x, w, bias, alpha, act):
        """act(alpha * x @ w + bias): bias / activation where the forward writes its result (x 2-D, or a channels-last 4-D activation
        whose NCHW flatten feeds the layer)."""
        return self._dense_fwd(x, w, bias, alpha, act)

    def dense_bwd_data(self, gy, w, alpha):
        return self._dense_bwd_data(gy, w, (gy.shape[0], w.shape[0]), alpha)

    def dense_bwd_weight(self, x, gy, alpha, out=None):
        return self._dense_bwd_weight(x, gy, alpha, out)

    @staticmethod
    def dense_nhwc_ok(x, out):
        if config.value("GS_NO_DENSE_NHWC"):   # measurement knob: the flatten copy + the plain kernels
            return False
        return x.dim() == 4 and x.is_contiguous(memory_format=CL) and out % 256 == 0 and (x.shape[1] * x.shape[2] * x.shape[3]) % 4 == 0 and x.shape[0] <= 16

    def dense_fwd_nhwc(self, x, w, alpha):
        return self._dense_fwd(x, w, None, alpha, _lib.ACT_NONE)

    def dense_bwd_data_nhwc(self, gy, w, x_shape, alpha):
        return self._dense_bwd_data(gy, w, x_shape, alpha)

    def dense_bwd_weight_nhwc(self, x, gy, alpha, out=None):
        return self._dense_bwd_weight(x, gy, alpha, out)

    def drop_deferred(self):
        """Forget every deferred job (a backward pass that raised in the middle of a capture: capture.Capture._abandon_capture)."""
        self._pending, self._folds = None, None
        self._seen, self._complete = None, None

    def embedding_fwd(self, idx, w, alpha, dtype):
        w = _f32c(w)
        idx = idx.contiguous()
        b = idx.shape[0]
        rows, units = w.shape
        y = torch.empty((b, units), dtype=dtype, device=w.device)
        _lib.check(self.lib.gs_embedding_fwd(idx.data_ptr(), w.data_ptr(), y.data_ptr(), b, rows, units, float(alpha), _dt(y), _stream()),
                   "gs_embedding_fwd")
        return y

    def embedding_onehot_fwd(self, labels, w, alpha):
        """(y, idx): the rows of w selected by the first maximum of each one-hot row, and those indices (for embedding_bwd)."""
        w = _f32c(w)
        labels = labels.contiguous()
        b, rows = labels.shape
        units = w.shape[1]
        assert rows == w.shape[0]
        y = torch.empty((b, units), dtype=labels.dtype, device=w.device)
        idx = torch.empty((b,), dtype=torch.int64, device=w.device)
        _lib.check(self.lib.gs_embedding_onehot_fwd(labels.data_ptr(), w.data_ptr(), y.data_ptr(), idx.data_ptr(), b, rows, units, float(alpha), _dt(labels),
                                                    _stream()), "gs_embedding_onehot_fwd")
        return y, idx

    def embedding_bwd(self, idx, gy, rows, alpha):
        gy = _act(gy)
        idx = idx.contiguous()
        b, units = gy.shape
        gw = torch.empty((rows, units), dtype=torch.float32, device=gy.device)
        _lib.check(self.lib.gs_embedding_bwd(idx.data_ptr(), gy.data_ptr(), gw.data_ptr(), b, rows, units, float(alpha), _dt(gy), _stream()),
                   "gs_embedding_bwd")
        return gw

    # ------------------------------------------------------------------ bias / activations
    def bias_act_fwd(self, x, bias, act):
        x = _act(x)
        p, c = _rows_cols(x)
        y = torch.empty_like(x)
        bp = None
        if bias is not None:
            bias = _f32c(bias)
            bp = bias.data_ptr()
        _lib.check(self.lib.gs_bias_act_fwd(x.data_ptr(), bp, y.data_ptr(), p, c, act, _dt(x), _stream()), "gs_bias_act_fwd")
        return y

    # the generator's first block: dense units (channel-major) <-> channels-last activation, in the bias / activation pass (gansynth_hip.h)
    def units_bias_act_to_nhwc(self, y, bias, c, h, w, act, mask=None):
        y = _act(y)
        n = y.shape[0]
        assert y.dim() == 2 and y.shape[1] == c * h * w
        z = torch.empty((n, c, h, w), dtype=y.dtype, device=y.device, memory_format=CL)
        bp = mp = None
        if bias is not None:
            bias = _f32c(bias)
            bp = bias.data_ptr()
        if mask is not None:
            mask = _match(mask, z)
            mp = mask.data_ptr()
        _lib.check(self.lib.gs_units_bias_act_to_nhwc(y.data_ptr(), bp, mp, z.data_ptr(), n, c, h * w, int(act), _dt(y), _stream()), "gs_units_bias_act_to_nhwc")
        return z

    def nhwc_act_bwd_to_units(self, g, z, act):
        z = _act(z)
        g = _match(g, z)
        n, c, h, w = z.shape
        gu = torch.empty((n, c * h * w), dtype=z.dtype, device=z.device)
        _lib.check(self.lib.gs_nhwc_act_bwd_to_units(g.data_ptr(), z.data_ptr(), gu.data_ptr(), n, c, h * w, int(act), _dt(z), _stream()), "gs_nhwc_act_bwd_to_units")
        return gu

    def act_bwd(self, g, y, act):
        y = _act(y)
        g = _match(g, y)
        gx = torch.empty_like(y)
        _lib.check(self.lib.gs_act_bwd(g.data_ptr(), y.data_ptr(), gx.data_ptr(), y.numel(), act, _dt(y), _stream()), "gs_act_bwd")
        return gx

    def act_bwd_bias(self, g, y, act, out=None):
        """(gx, gb): activation backward and the bias gradient in one pass (gb added into `out` when given)."""
        y = _act(y)
        g = _match(g, y)
        p, c = _rows_cols(y)
        gx = torch.empty_like(y)
        gb = torch.empty((c,), dtype=torch.float32, device=y.device) if out is None else out
        part = self._partial_rows(_lib.BIAS_FROM_ACT_BWD, p, c, _dt(y), out)
        ws = part if part is not None else _ws(self.lib.gs_channel_sum_workspace_bytes(p, c), y.device)
        flags = (0 if out is None else 1) | (_lib.SUM_PARTIALS if part is not None else 0)
        with self._adds_into(out if part is None else None):   # (partial rows left for the batched fold: `out` is not touched now)
            _lib.check(self.lib.gs_act_bwd_bias(g.data_ptr(), y.data_ptr(), gx.data_ptr(), gb.data_ptr(), p, c, act, flags,
                                                _dt(y), ws.data_ptr(), ws.numel() * ws.element_size(), _stream()), "gs_act_bwd_bias")
        return gx, gb

    def tanh_bwd_bwd(self, gg, g, y):
        y = _act(y)
        gg, g = _match(gg, y), _match(g, y)
        out = torch.empty_like(y)
        _lib.check(self.lib.gs_tanh_bwd_bwd(gg.data_ptr(), g.data_ptr(), y.data_ptr(), out.data_ptr(), y.numel(), _dt(y), _stream()),
                   "gs_tanh_bwd_bwd")
        return out

    def channel_sum(self, g, out=None):
        g = _act(g)
        p, c = _rows_cols(g)
        res = torch.empty((c,), dtype=torch.float32, device=g.device) if out is None else out
        part = self._partial_rows(_lib.BIAS_FROM_CHANNEL_SUM, p, c, _dt(g), out)
        ws = part if part is not None else _ws(self.lib.gs_channel_sum_workspace_bytes(p, c), g.device)
        flags = (0 if out is None else 1) | (_lib.SUM_PARTIALS if part is not None else 0)
        with self._adds_into(out if part is None else None):
            _lib.check(self.lib.gs_channel_sum(g.data_ptr(), res.data_ptr(), p, c, flags, _dt(g), ws.data_ptr(), ws.numel() * ws.element_size(),
                                               _stream()), "gs_channel_sum")
        return res

    def pixel_norm_fwd(self, x, eps):
        x = _act(x)
        p, c = _rows_cols(x)
        y = torch.empty_like(x)
        _lib.check(self.lib.gs_pixel_norm_fwd(x.data_ptr(), y.data_ptr(), p, c, float(eps), _dt(x), _stream()), "gs_pixel_norm_fwd")
        return y

    norm_bwd_sums_bias = True   # pixel_norm_bwd(bias_out=...) exists (functional._ConvBiasActNorm)

    def norm_bwd_bias_ok(self, c, dtype=torch.float32):
        """Can pixel_norm_bwd(bias_out=...) take rows of `c` channels?  (gs_pixel_norm_bwd_fused_bias: a power of two in 4..1024 --
        the library's own answer: gs_bias_partial_rows is 0 for the shapes that kernel rejects.)"""
        return self.lib.gs_bias_partial_rows(_lib.BIAS_FROM_PIXEL_NORM_BWD, 1, int(c), GS_F32 if dtype == torch.float32 else GS_BF16) > 0

    def pixel_norm_bwd(self, g, x, eps, act=0, pre_act=0, addend=None, bias_out=None):
        """gx = (pixel_norm_bwd(g * pre_act'(x), x) + addend) * act'(x)   (x: an activation output; see gs_pixel_norm_bwd_fused).
        `bias_out` (fp32 [c], contiguous): the same pass adds sum_pixels gx into it."""
        x = _act(x)
        g = _match(g, x)
        p, c = _rows_cols(x)
        gx = torch.empty_like(x)
        ap = None
        if addend is not None:
            addend = _match(addend, x)
            ap = addend.data_ptr()
        if bias_out is not None:
            assert bias_out.dtype == torch.float32 and bias_out.is_contiguous() and bias_out.numel() == c
            part = self._partial_rows(_lib.BIAS_FROM_PIXEL_NORM_BWD, p, c, _dt(x), bias_out)
            ws = part if part is not None else _ws(self.lib.gs_pixel_norm_bwd_bias_workspace_bytes(p, c, _dt(x)), x.device)
            with self._adds_into(bias_out if part is None else None):
                _lib.check(self.lib.gs_pixel_norm_bwd_fused_bias(g.data_ptr(), x.data_ptr(), ap, gx.data_ptr(), bias_out.data_ptr(), p, c, float(eps), int(pre_act),
                                                                 int(act), 1 | (_lib.SUM_PARTIALS if part is not None else 0), _dt(x), ws.data_ptr(),
                                                                 ws.numel() * ws.element_size(), _stream()), "gs_pixel_norm_bwd_fused_bias")
            return gx
        _lib.check(self.lib.gs_pixel_norm_bwd_fused(g.data_ptr(), x.data_ptr(), ap, gx.data_ptr(), p, c, float(eps), int(pre_act), int(act), _dt(x),
                                                    _stream()), "gs_pixel_norm_bwd_fused")
        return gx

    def pixel_norm_bwd_bwd(self, gg, g, x, eps, pre_act=0, with_g=False):
        """d<gg', pixel_norm_bwd(g, x)>/dx with gg' = gg * pre_act'(x); with_g: also pixel_norm_bwd(gg', x) (same pass) -> (out, out_g)."""
        x = _act(x)
        gg, g = _match(gg, x), _match(g, x)
        p, c = _rows_cols(x)
        out = torch.empty_like(x)
        out_g = torch.empty_like(x) if with_g else None
        _lib.check(self.lib.gs_pixel_norm_bwd_bwd_fused(gg.data_ptr(), g.data_ptr(), x.data_ptr(), out.data_ptr(), None if out_g is None else out_g.data_ptr(),
                                                        p, c, float(eps), int(pre_act), _dt(x), _stream()), "gs_pixel_norm_bwd_bwd_fused")
        return (out, out_g) if with_g else out

    # --------------------------------------------------------------------- up / down scale
    def upscale2d(self, x, fy, fx, scale):
        x = _act(x)
        n, c, h, w = x.shape
        y = _empty_like_act((n, c, h * fy, w * fx), x)
        _lib.check(self.lib.gs_upscale2d(x.data_ptr(), y.data_ptr(), n, h, w, c, fy, fx, float(scale), _dt(x), _stream()), "gs_upscale2d")
        return y

    def blocksum2d(self, x, fy, fx, scale):
        x = _act(x)
        n, c, h, w = x.shape
        y = _empty_like_act((n, c, h // fy, w // fx), x)
        _lib.check(self.lib.gs_blocksum2d(x.data_ptr(), y.data_ptr(), n, h, w, c, fy, fx, float(scale), _dt(x), _stream()), "gs_blocksum2d")
        return y

    # ------------------------------------------------------------------------ batch stddev
    # (`sub`: x is `sub` batches concatenated along axis 0 -- the statistic of ops.py:336-348 within each: one call per sub-batch on its slab)
    def batch_stddev_fwd(self, x, eps, sub=1):
        x = _act(x)
        n, c, h, w = x.shape
        y = _empty_like_act((n, 1, h, w), x)
        m, es = n // sub, x.element_size()
        for s in range(sub):
            _lib.check(self.lib.gs_batch_stddev_fwd(x.data_ptr() + s * m * c * h * w * es, y.data_ptr() + s * m * h * w * es, m, h * w, c, float(eps), _dt(x),
                                                    _stream()), "gs_batch_stddev_fwd")
        return y

    def batch_stddev_bwd(self, gy, x, eps, addend=None, sub=1):
        """d batch_stddev(x) / d x applied to gy, plus `addend` (another gradient into x) in the same pass."""
        x = _act(x)
        n, c, h, w = x.shape
        gy = _act(gy.to(x.dtype))
        gx = torch.empty_like(x)
        if addend is not None:
            addend = _match(addend, x)
        m, es = n // sub, x.element_size()
        for s in range(sub):
            ox, oy = s * m * c * h * w * es, s * m * h * w * es
            _lib.check(self.lib.gs_batch_stddev_bwd(gy.data_ptr() + oy, x.data_ptr() + ox, None if addend is None else addend.data_ptr() + ox, gx.data_ptr() + ox,
                                                    m, h * w, c, float(eps), _dt(x), _stream()), "gs_batch_stddev_bwd")
        return gx

    def batch_stddev_bwd_bwd(self, ggx, gy, x, eps, sub=1):
        x = _act(x)
        n, c, h, w = x.shape
        ggx = _match(ggx, x)
        gy = _act(gy.to(x.dtype))
        ggy = torch.empty_like(gy)
        gx2 = torch.empty_like(x)
        m, es = n // sub, x.element_size()
        for s in range(sub):
            ox, oy = s * m * c * h * w * es, s * m * h * w * es
            _lib.check(self.lib.gs_batch_stddev_bwd_bwd(ggx.data_ptr() + ox, gy.data_ptr() + oy, x.data_ptr() + ox, ggy.data_ptr() + oy, gx2.data_ptr() + ox,
                                                        m, h * w, c, float(eps), _dt(x), _stream()), "gs_batch_stddev_bwd_bwd")
        return ggy, gx2

    # ------------------------------------------------------------------- misc elementwise
    def axpby(self, a, b, ca, cb):
        a = _act(a)
        b = _match(b, a)
        out = torch.empty_like(a)
        if hasattr(ca, "owner") or hasattr(cb, "owner"):   # functional.DeviceLerp.Coef: coefficients read from a device table
            if not (hasattr(ca, "owner") and hasattr(cb, "owner") and ca.owner is cb.owner):
                raise TypeError("axpby: device coefficients must come from one DeviceLerp table")
            _lib.check(self.lib.gs_axpby_dev(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), ca.owner.table.data_ptr(), ca.index, cb.index,
                                             _dt(a), _stream()), "gs_axpby_dev")
            return out
        _lib.check(self.lib.gs_axpby(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), float(ca), float(cb), _dt(a), _stream()), "gs_axpby")
        return out

    def sumsq_rows(self, x):
        x = _act(x)
        rows = x.shape[0]
        out = torch.empty((rows,), dtype=torch.float32, device=x.device)
        ws = _ws(self.lib.gs_sumsq_rows_workspace_bytes(rows), x.device)
        _lib.check(self.lib.gs_sumsq_rows(x.data_ptr(), out.data_ptr(), rows, x.numel() // rows, _dt(x), ws.data_ptr(), ws.numel(), _stream()), "gs_sumsq_rows")
        return out

    def row_scale(self, x, s, alpha=1.0):
        """out[r] = alpha * s[r] * x[r]."""
        x = _act(x)
        s = _f32c(s)
        rows = x.shape[0]
        out = torch.empty_like(x)
        _lib.check(self.lib.gs_row_scale(x.data_ptr(), s.data_ptr(), float(alpha), out.data_ptr(), rows, x.numel() // rows, _dt(x), _stream()), "gs_row_scale")
        return out

    def gan_d_loss(self, real_logits, fake_logits, labels, penalty, penalty_weight=1.0, out=None):
        """(loss, g_real_logits, g_fake_logits, g_penalty): mean of softplus(-r) + softplus(f) + penalty_weight * penalty and its gradients, one launch.
        Either logits tensor may be None (the other half of the sum is then another launch: see include/gansynth_hip.h)."""
        real_logits = None if real_logits is None else _act(real_logits)
        fake_logits = None if fake_logits is None else _act(fake_logits)
        ref = real_logits if real_logits is not None else fake_logits
        labels = _match(labels, ref)
        n, c = ref.shape
        loss = torch.empty((), dtype=torch.float32, device=ref.device)
        if out is None:
            g_real = None if real_logits is None else torch.empty_like(real_logits)
            g_fake = None if fake_logits is None else torch.empty_like(fake_logits)
        else:
            g_real, g_fake = out
        pp = g_pen = None
        if penalty is not None:
            penalty = _f32c(penalty)
            pp = penalty.data_ptr()
            g_pen = torch.empty((n,), dtype=torch.float32, device=ref.device)
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(self.lib.gs_gan_d_loss(ptr(real_logits), ptr(fake_logits), labels.data_ptr(), pp, float(penalty_weight), n, c, loss.data_ptr(),
                                          ptr(g_real), ptr(g_fake), ptr(g_pen), _dt(ref), _stream()), "gs_gan_d_loss")
        return loss, g_real, g_fake, g_pen

    def gan_g_loss(self, fake_logits, labels, sumsq, weight, eps):
        """(loss, g_fake_logits, g_sumsq): mean of softplus(-f) + weight / (sumsq + eps) and its gradients, one launch.  `fake_logits` None:
        the mode-seeking half alone."""
        sp = gp = None
        g_sumsq = None
        if sumsq is not None:
            sumsq = _f32c(sumsq)
            g_sumsq = torch.empty_like(sumsq)
            sp, gp = sumsq.data_ptr(), g_sumsq.data_ptr()
        if fake_logits is None:
            loss = torch.empty((), dtype=torch.float32, device=sumsq.device)
            _lib.check(self.lib.gs_gan_g_loss(None, None, sp, float(weight), float(eps), sumsq.numel(), 1, loss.data_ptr(), None, gp, _lib.GS_F32, _stream()),
                       "gs_gan_g_loss")
            return loss, None, g_sumsq
        fake_logits = _act(fake_logits)
        labels = _match(labels, fake_logits)
        n, c = fake_logits.shape
        loss = torch.empty((), dtype=torch.float32, device=fake_logits.device)
        g_fake = torch.empty_like(fake_logits)
        _lib.check(self.lib.gs_gan_g_loss(fake_logits.data_ptr(), labels.data_ptr(), sp, float(weight), float(eps), n, c, loss.data_ptr(), g_fake.data_ptr(), gp,
                                          _dt(fake_logits), _stream()), "gs_gan_g_loss")
        return loss, g_fake, g_sumsq

    def adam_tf_step(self, p, g, m, v, lr_t, beta1, beta2, eps, grad_scale=1.0, refresh=True, zero_grad=False):
        """`refresh=False`: the caller updates a buffer range by range (gradient buckets) and refreshes the operands once.
        `zero_grad`: g is cleared behind the update (the next run accumulates from zero without a fill pass)."""
        for t in (p, g, m, v):
            assert t.dtype == torch.float32 and t.is_contiguous()
        fn = self.lib.gs_adam_tf_step_zero_grad if zero_grad else self.lib.gs_adam_tf_step
        _lib.check(fn(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr_t), float(beta1),
                      float(beta2), float(eps), float(grad_scale), _stream()), "gs_adam_tf_step")
        if refresh:
            self.invalidate_weights(p)  # parameter values changed: cached kernel operands of that buffer are stale ...
            self.refresh_weights(p)     # ... and are rebuilt here in one launch

    def adam_tf_step_dev(self, p, g, m, v, lr_t_ptr, beta1, beta2, eps, grad_scale=1.0, refresh=True, zero_grad=False):
        """adam_tf_step with lr_t read from device memory when the launch EXECUTES (`lr_t_ptr`: address of one fp32; negative = no step):
        the form a captured graph can hold.  `refresh`: the prepared operands of every weight in `p` are rebuilt behind it, unconditionally
        -- inside a capture the host-side staleness stamps describe the capture pass, not the replays."""
        for t in (p, g, m, v):
            assert t.dtype == torch.float32 and t.is_contiguous()
        _lib.check(self.lib.gs_adam_tf_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), int(lr_t_ptr), float(beta1),
                                                float(beta2), float(eps), float(grad_scale), 1 if zero_grad else 0, _stream()), "gs_adam_tf_step_dev")
        if refresh:
            self.invalidate_weights(p)
            self.refresh_weights(p)

    def ema_step(self, shadow, p, one_minus_decay):
        """tf.train.ExponentialMovingAverage's update of a flat fp32 buffer: shadow -= (shadow - p) * one_minus_decay (gs_ema_step)."""
        for t in (shadow, p):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert shadow.numel() == p.numel()
        _lib.check(self.lib.gs_ema_step(shadow.data_ptr(), p.data_ptr(), p.numel(), float(one_minus_decay), _stream()), "gs_ema_step")
        self.ema_steps += 1

    def ema_step_dev(self, shadow, p, one_minus_ptr):
        """ema_step with the scalar read from device memory when the launch EXECUTES (`one_minus_ptr`: address of one fp32; negative = no
        step pending): the form a captured graph can hold, as adam_tf_step_dev."""
        for t in (shadow, p):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert shadow.numel() == p.numel()
        _lib.check(self.lib.gs_ema_step_dev(shadow.data_ptr(), p.data_ptr(), p.numel(), int(one_minus_ptr), _stream()), "gs_ema_step_dev")
        self.ema_steps_dev += 1

    def swap_(self, a, b):
        """a and b (flat fp32, same size) exchange their contents in place, bit for bit (gs_swap_f32).  The caller invalidates and
        refreshes prepared operands where one of them is a parameter buffer."""
        for t in (a, b):
            assert t.dtype == torch.float32 and t.is_contiguous()
        assert a.numel() == b.numel()
        _lib.check(self.lib.gs_swap_f32(a.data_ptr(), b.data_ptr(), a.numel(), _stream()), "gs_swap_f32")

    # ------------------------------------------------------------------- more than one stream
    def stream_guard(self):
        """`with K.stream_guard():` -- every tensor argument of every kernel-layer call made inside is marked with the stream the call
        runs on (Tensor.record_stream: a no-op for the stream the tensor was allocated on).  A run captured with forked branches
        (models.GANSynth._branch) reads tensors on a stream other than their own; torch's caching allocator would otherwise hand a freed
        block straight back to ITS stream while the other stream's kernel is still reading it.  Inside a stream capture a marked block
        is not reused until the capture ends.  Costs host time at capture only; the wrappers exist while the context does."""
        return _StreamGuard(self)

    # --------------------------------------------------------------------------- profiling
    # ------------------------------------------------------------ pitch classifier (networks.ResNet: inference only)
    def weight_standardize(self, w, eps, out=None):
        """ops.py:53-66 on an fp32 HWIO / [in, out] weight: per output channel over everything else."""
        w = _f32c(w)
        out = torch.empty_like(w) if out is None else out
        co = w.shape[-1]
        _lib.check(self.lib.gs_weight_standardize(w.data_ptr(), out.data_ptr(), w.numel() // co, co, float(eps), _stream()), "gs_weight_standardize")
        return out

    def conv2d_fwd_bias_ws(self, x, w, bias, ksize, stride, ws, prepared):
        """gs_conv_fwd with alpha = 1, no activation, and a workspace the CALLER keeps with its weight (`prepared`: it still
        holds the re-laid operand of this weight)."""
        x = _act(x)
        n, ci, h, wd = x.shape
        co = w.shape[3]
        y = _empty_like_act((n, co, h // stride, wd // stride), x)
        c = _lib.GsConv(n, h, wd, ci, co, ksize, stride, 0, _dt(x), int(prepared), 1.0, ws.data_ptr(), ws.numel())
        _lib.check(self.lib.gs_conv_fwd(c, x.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(), _lib.ACT_NONE, y.data_ptr(), None, 0.0, _stream()),
                   "gs_conv_fwd")
        return y

    def conv2d_fwd_workspace(self, x_shape, co, ksize, stride, dtype):
        n, ci, h, wd = x_shape
        return _ws(self.lib.gs_conv_workspace_bytes(_lib.GsConv(n, h, wd, ci, co, ksize, stride, 0, dtype), _lib.CONV_FWD), torch.device("cuda"))

    def resnet_stem_pool(self, x, w, bias, want_stem=False, want_pool=True):
        """(stem, pool): conv 7x7 / 2 + bias (TF SAME) and max pool 3x3 / 2 of it in one kernel; stem is None unless asked for."""
        x = _act(x)
        n, c, h, wd = x.shape
        co = w.shape[3]
        stem = _empty_like_act((n, co, h // 2, wd // 2), x) if want_stem else None
        pool = _empty_like_act((n, co, h // 4, wd // 4), x) if want_pool else None
        _lib.check(self.lib.gs_resnet_stem_pool(x.data_ptr(), _f32c(w).data_ptr(), None if bias is None else _f32c(bias).data_ptr(),
                                                None if stem is None else stem.data_ptr(), None if pool is None else pool.data_ptr(),
                                                n, h, wd, co, _dt(x), _stream()), "gs_resnet_stem_pool")
        return stem, pool

    def max_pool2d(self, x):
        x = _act(x)
        n, c, h, wd = x.shape
        y = _empty_like_act((n, c, h // 2, wd // 2), x)
        _lib.check(self.lib.gs_max_pool2d(x.data_ptr(), y.data_ptr(), n, h, wd, c, _dt(x), _stream()), "gs_max_pool2d")
        return y

    def conv1x1_fwd(self, x, w, stride):
        """x[:, :, ::stride, ::stride] through the 1x1 weight w ([1, 1, ci, co] or [ci, co]), no bias."""
        x = _act(x)
        n, ci, h, wd = x.shape
        co = w.shape[-1]
        y = _empty_like_act((n, co, h // stride, wd // stride), x)
        _lib.check(self.lib.gs_conv1x1_fwd(x.data_ptr(), _f32c(w).data_ptr(), y.data_ptr(), n, h, wd, ci, co, int(stride), _dt(x), _stream()),
                   "gs_conv1x1_fwd")
        return y

    def group_norm_stats(self, x, groups, eps, addend=None):
        """(stats [n, groups, 2] = (mean, rstd), s): the statistics of s = x (+ addend, written as it is read)."""
        x = _act(x)
        n, c, h, wd = x.shape
        s = x
        if addend is not None:
            addend = _act(addend)
            assert addend.shape == x.shape and addend.dtype == x.dtype
            s = _empty_like_act(tuple(x.shape), x)
        stats = torch.empty((n, groups, 2), dtype=torch.float32, device=x.device)
        ws = _ws(self.lib.gs_group_norm_workspace_bytes(n, h * wd, c, groups), x.device)
        _lib.check(self.lib.gs_group_norm_stats(x.data_ptr(), None if addend is None else addend.data_ptr(), None if addend is None else s.data_ptr(),
                                                stats.data_ptr(), n, h * wd, c, groups, float(eps), _dt(x), ws.data_ptr(), ws.numel(), _stream()),
                   "gs_group_norm_stats")
        return stats, s

    def group_norm_apply(self, x, stats, gamma, beta, relu):
        x = _act(x)
        n, c, h, wd = x.shape
        y = _empty_like_act(tuple(x.shape), x)
        _lib.check(self.lib.gs_group_norm_apply(x.data_ptr(), stats.data_ptr(), _f32c(gamma).data_ptr(), _f32c(beta).data_ptr(), y.data_ptr(),
                                                n, h * wd, c, stats.shape[1], int(bool(relu)), _dt(x), _stream()), "gs_group_norm_apply")
        return y

    def group_norm_relu_mean(self, x, stats, gamma, beta):
        """fp32 [n, c]: mean over H, W of relu(group_norm(x))."""
        x = _act(x)
        n, c, h, wd = x.shape
        out = torch.empty((n, c), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.gs_group_norm_relu_mean(x.data_ptr(), stats.data_ptr(), _f32c(gamma).data_ptr(), _f32c(beta).data_ptr(), out.data_ptr(),
                                                    n, h * wd, c, stats.shape[1], _dt(x), _stream()), "gs_group_norm_relu_mean")
        return out

    # ------------------------------------------------------------ pitch classifier, training (networks.ResNet.forward_backward)
    def _gn_bwd_outputs(self, x, dgamma, dbeta):
        c = x.shape[1]
        if dgamma is None:
            dgamma = torch.empty((c,), dtype=torch.float32, device=x.device)
        if dbeta is None:
            dbeta = torch.empty((c,), dtype=torch.float32, device=x.device)
        for t in (dgamma, dbeta):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == c
        return dgamma, dbeta

    def group_norm_relu_bwd(self, x, stats, gamma, beta, gy, addend=None, dgamma=None, dbeta=None):
        """(dx [+ addend], dgamma, dbeta) of y = relu(group_norm(x)) from the upstream gradient gy; `dgamma` / `dbeta` (fp32, c
        elements): written in place."""
        x, gy = _act(x), _act(gy)
        n, c, h, wd = x.shape
        assert gy.shape == x.shape and gy.dtype == x.dtype
        if addend is not None:
            addend = _act(addend)
            assert addend.shape == x.shape and addend.dtype == x.dtype
        dgamma, dbeta = self._gn_bwd_outputs(x, dgamma, dbeta)
        dx = _empty_like_act(tuple(x.shape), x)
        groups = stats.shape[1]
        ws = _ws(self.lib.gs_group_norm_bwd_workspace_bytes(n, h * wd, c, groups), x.device)
        _lib.check(self.lib.gs_group_norm_relu_bwd(x.data_ptr(), stats.data_ptr(), _f32c(gamma).data_ptr(), _f32c(beta).data_ptr(), gy.data_ptr(),
                                                   None if addend is None else addend.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                                   n, h * wd, c, groups, 0, _dt(x), ws.data_ptr(), ws.numel(), _stream()), "gs_group_norm_relu_bwd")
        return dx, dgamma, dbeta

    def group_norm_relu_mean_bwd(self, x, stats, gamma, beta, gfeatures, dgamma=None, dbeta=None):
        """The backward of group_norm_relu_mean from d features [n, c] (fp32)."""
        x, gfeatures = _act(x), _f32c(gfeatures)
        n, c, h, wd = x.shape
        assert tuple(gfeatures.shape) == (n, c)
        dgamma, dbeta = self._gn_bwd_outputs(x, dgamma, dbeta)
        dx = _empty_like_act(tuple(x.shape), x)
        groups = stats.shape[1]
        ws = _ws(self.lib.gs_group_norm_bwd_workspace_bytes(n, h * wd, c, groups), x.device)
        _lib.check(self.lib.gs_group_norm_relu_mean_bwd(x.data_ptr(), stats.data_ptr(), _f32c(gamma).data_ptr(), _f32c(beta).data_ptr(),
                                                        gfeatures.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), n, h * wd, c, groups, 0,
                                                        _dt(x), ws.data_ptr(), ws.numel(), _stream()), "gs_group_norm_relu_mean_bwd")
        return dx, dgamma, dbeta

    def weight_standardize_table(self, rows):
        """Device table for weight_standardize_batch / _bwd_batch.  rows: (w, out, rstd, gout, gw) fp32 contiguous tensors per weight
        ([..., co]; rstd [co]; gout / gw may be None for a forward-only table).  The table keeps its tensors alive."""
        arr = (_lib.GsWsDesc * len(rows))()
        max_co = 0
        for d, (w, out, rstd, gout, gw) in zip(arr, rows):
            co = w.shape[-1]
            for t in (w, out, rstd, gout, gw):
                assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
            assert out.shape == w.shape and rstd.numel() == co and (gout is None or gout.shape == w.shape) and (gw is None or gw.shape == w.shape)
            d.w, d.out, d.rstd = w.data_ptr(), out.data_ptr(), rstd.data_ptr()
            d.gout, d.gw = (None if gout is None else gout.data_ptr()), (None if gw is None else gw.data_ptr())
            d.fan_in, d.co = w.numel() // co, co
            max_co = max(max_co, co)
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        return dict(table=host.to(rows[0][0].device), n=len(rows), max_co=max_co, rows=rows, backward=all(r[3] is not None and r[4] is not None for r in rows))

    def weight_standardize_batch(self, table, eps):
        _lib.check(self.lib.gs_weight_standardize_batch(table["table"].data_ptr(), table["n"], table["max_co"], float(eps), _stream()),
                   "gs_weight_standardize_batch")

    def weight_standardize_bwd_batch(self, table):
        """gw = the gradient through the standardisation of every weight of the table, from gout (cleared behind the read)."""
        assert table["backward"], "the table was built without gradient buffers"
        _lib.check(self.lib.gs_weight_standardize_bwd_batch(table["table"].data_ptr(), table["n"], table["max_co"], _stream()),
                   "gs_weight_standardize_bwd_batch")

    def max_pool2d_bwd(self, x, gy):
        """Gradient of the 3x3 / 2 SAME max pool of x (any h, w): a window's gradient goes to its first maximum."""
        x, gy = _act(x), _act(gy)
        n, c, h, wd = x.shape
        assert tuple(gy.shape) == (n, c, (h + 1) // 2, (wd + 1) // 2) and gy.dtype == x.dtype
        gx = _empty_like_act(tuple(x.shape), x)
        _lib.check(self.lib.gs_max_pool2d_bwd(x.data_ptr(), gy.data_ptr(), gx.data_ptr(), n, h, wd, c, _dt(x), _stream()), "gs_max_pool2d_bwd")
        return gx

    def resnet_stem_bwd_weight(self, x, gstem, out=None, bias_out=None):
        """(gw [7, 7, 2, 64], gb [64]) of the stem conv from its input and the gradient of its output; `out` / `bias_out`: added into."""
        x, gstem = _act(x), _act(gstem)
        n, c, h, wd = x.shape
        co = gstem.shape[1]
        assert c == 2 and tuple(gstem.shape) == (n, co, h // 2, wd // 2) and gstem.dtype == x.dtype and (out is None) == (bias_out is None)
        gw = torch.empty((7, 7, 2, co), dtype=torch.float32, device=x.device) if out is None else out
        gb = torch.empty((co,), dtype=torch.float32, device=x.device) if bias_out is None else bias_out
        assert gw.is_contiguous() and gb.is_contiguous() and gw.dtype == gb.dtype == torch.float32
        ws = _ws(self.lib.gs_resnet_stem_bwd_weight_workspace_bytes(n, h, wd), x.device)
        _lib.check(self.lib.gs_resnet_stem_bwd_weight(x.data_ptr(), gstem.data_ptr(), gw.data_ptr(), gb.data_ptr(), n, h, wd, co, 0 if out is None else 1,
                                                      _dt(x), ws.data_ptr(), ws.numel(), _stream()), "gs_resnet_stem_bwd_weight")
        return gw, gb

    def conv1x1_bwd_data(self, gy, w, x_shape, stride, out=None):
        """gx [n, ci, h, w] of conv1x1_fwd; `out`: the gradient is ADDED into it at the sampled pixels (the other consumer's gradient
        is already there)."""
        gy = _act(gy)
        n, ci, h, wd = x_shape
        co = w.shape[-1]
        assert tuple(gy.shape) == (n, co, h // stride, wd // stride)
        gx = _empty_like_act((n, ci, h, wd), gy) if out is None else out
        assert gx.dtype == gy.dtype and tuple(gx.shape) == (n, ci, h, wd) and gx.is_contiguous(memory_format=CL)
        _lib.check(self.lib.gs_conv1x1_bwd_data(gy.data_ptr(), _f32c(w).data_ptr(), gx.data_ptr(), n, h, wd, ci, co, int(stride), 0 if out is None else 1,
                                                _dt(gy), _stream()), "gs_conv1x1_bwd_data")
        return gx

    def conv1x1_bwd_weight(self, x, gy, stride, out=None):
        """gw [1, 1, ci, co] of conv1x1_fwd; `out`: added into."""
        x, gy = _act(x), _act(gy)
        n, ci, h, wd = x.shape
        co = gy.shape[1]
        assert tuple(gy.shape) == (n, co, h // stride, wd // stride) and gy.dtype == x.dtype
        gw = torch.empty((1, 1, ci, co), dtype=torch.float32, device=x.device) if out is None else out
        assert gw.is_contiguous() and gw.dtype == torch.float32 and gw.numel() == ci * co
        ws = _ws(self.lib.gs_conv1x1_bwd_weight_workspace_bytes(n, h, wd, ci, co, int(stride)), x.device)
        _lib.check(self.lib.gs_conv1x1_bwd_weight(x.data_ptr(), gy.data_ptr(), gw.data_ptr(), n, h, wd, ci, co, int(stride), 0 if out is None else 1,
                                                  _dt(x), ws.data_ptr(), ws.numel(), _stream()), "gs_conv1x1_bwd_weight")
        return gw

    def softmax_xent(self, logits, labels, want_grad=True):
        """(loss [1] fp32 = mean softmax cross-entropy, dlogits or None, correct [1] int32 = rows whose argmax matches the labels')."""
        logits, labels = _f32c(logits), _f32c(labels)
        n, c = logits.shape
        assert labels.shape == logits.shape
        loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
        correct = torch.empty((1,), dtype=torch.int32, device=logits.device)
        dlogits = torch.empty_like(logits) if want_grad else None
        _lib.check(self.lib.gs_softmax_xent(logits.data_ptr(), labels.data_ptr(), loss.data_ptr(), None if dlogits is None else dlogits.data_ptr(),
                                            correct.data_ptr(), n, c, _stream()), "gs_softmax_xent")
        return loss, dlogits, correct

    def momentum_tf_step(self, p, g, accum, lr, momentum, use_nesterov, weight_decay=0.0, decay_range=(0, 0), zero_grad=True, want_l2=True):
        """tf.train.MomentumOptimizer over a flat buffer, the L2 term's gradient (weight_decay * p on decay_range) folded in; returns
        sum p^2 / 2 of that range at the pre-update values ([1] fp32) or None.  zero_grad=False leaves g as it came: the kernel adds the
        L2 term in registers and stores nothing back to g."""
        for t in (p, g, accum):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel()
        l2 = torch.empty((1,), dtype=torch.float32, device=p.device) if want_l2 else None
        ws = _ws(self.lib.gs_momentum_workspace_bytes(p.numel()), p.device)
        _lib.check(self.lib.gs_momentum_tf_step(p.data_ptr(), g.data_ptr(), accum.data_ptr(), p.numel(), int(decay_range[0]), int(decay_range[1]),
                                                float(weight_decay), float(lr), float(momentum), 1 if use_nesterov else 0, 1 if zero_grad else 0,
                                                None if l2 is None else l2.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "gs_momentum_tf_step")
        return l2

    def summary_image_u8(self, x, count=4):
        """tf.summary.image's 8-bit rule (include/gansynth_hip.h) on the first min(B, count) images of x: [B, H, W], or [B, 2, H, W]
        channels-last (both planes from one pass).  Returns uint8 [n, C, H, W], contiguous."""
        n = min(int(x.shape[0]), int(count))
        x = _act(x[:n])
        if x.dim() == 4:
            _, c, h, w = x.shape
        else:
            (_, h, w), c = x.shape, 1
        out = torch.empty((n, c, h, w), dtype=torch.uint8, device=x.device)
        ws = _ws(self.lib.gs_summary_image_u8_workspace_bytes(n, h * w, c), x.device)
        _lib.check(self.lib.gs_summary_image_u8(x.data_ptr(), out.data_ptr(), n, h * w, c, _dt(x), ws.data_ptr(), ws.numel(), _stream()),
                   "gs_summary_image_u8")
        return out

    def summary_audio_s16(self, x, count=4):
        """TF's FloatToInt16Sample on the first min(B, count) rows of x [B, L] (any row stride): int16 [n, L]."""
        n = min(int(x.shape[0]), int(count))
        x = x[:n]
        length = int(x.shape[1])
        if x.stride(1) != 1 or (n > 1 and x.stride(0) < length):
            x = x.contiguous()
        out = torch.empty((n, length), dtype=torch.int16, device=x.device)
        _lib.check(self.lib.gs_summary_audio_s16(x.data_ptr(), out.data_ptr(), n, length, int(x.stride(0)) if n > 1 else length, _dt(x), _stream()),
                   "gs_summary_audio_s16")
        return out

    def _note_mix(self, channels, waves, table, total, normalize, want_pcm):
        """note_mix (channels 1: out [total], pcm [total]) and note_mix_stereo (2: out [2, total] with rows on 16 bytes, pcm [total, 2])."""
        name = "note_mix" if channels == 1 else "note_mix_stereo"
        if waves.dim() != 2 or waves.dtype != torch.float32:
            raise ValueError(f"{name}: waves must be [rows, L] fp32 (got {tuple(waves.shape)} {waves.dtype})")
        rows, length = int(waves.shape[0]), int(waves.shape[1])
        total = int(total)
        arr = (note_mix_table if channels == 1 else note_mix_stereo_table)(table, rows, length, total)
        if waves.stride(1) != 1 or (rows > 1 and waves.stride(0) < length):
            waves = waves.contiguous()
        notes = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(waves.device)   # uploaded once
        stride = (total + 3) // 4 * 4
        out = torch.empty((total,) if channels == 1 else (2, stride), dtype=torch.float32, device=waves.device)
        pcm = torch.empty((total,) if channels == 1 else (total, 2), dtype=torch.int16, device=waves.device) if want_pcm else None
        peak = torch.empty((1,), dtype=torch.float32, device=waves.device)
        ws = _ws(getattr(self.lib, f"gs_{name}_workspace_bytes")(total), waves.device)
        _lib.check(getattr(self.lib, f"gs_{name}")(waves.data_ptr(), rows, length, int(waves.stride(0)) if rows > 1 else length, notes.data_ptr(),
                                                   len(arr), total, 1 if normalize else 0, out.data_ptr(), *(() if channels == 1 else (stride,)),
                                                   None if pcm is None else pcm.data_ptr(), peak.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                   f"gs_{name}")
        return (out if channels == 1 else out[:, :total]), pcm, peak

    def note_mix(self, waves, table, total, normalize=True, want_pcm=False):
        """gs_note_mix (include/gansynth_hip.h): the notes of `table` -- host rows (onset, hold, release, row, gain) -- mixed from the rows of
        waves [rows, L] fp32 into one clip.  -> (out [total] fp32, pcm [total] int16 or None, peak [1] fp32 = max |mix|); out is the mix
        divided by peak when `normalize` and peak > 1."""
        return self._note_mix(1, waves, table, total, normalize, want_pcm)

    def note_mix_stereo(self, waves, table, total, normalize=True, want_pcm=False):
        """gs_note_mix_stereo (include/gansynth_hip.h): the notes of `table` -- host rows (onset, hold, release, row, gain_l, gain_r) -- mixed
        from the rows of waves [rows, L] fp32 into two channels with ONE peak.  -> (out [2, total] fp32 -- a view of [2, S], S = total
        rounded up to 4, so that both rows start on 16 bytes --, pcm [total, 2] int16 or None, peak [1] fp32 = max |mix| over both
        channels); both channels are divided by peak when `normalize` and peak > 1."""
        return self._note_mix(2, waves, table, total, normalize, want_pcm)

    def note_mix_curves(self, waves, table, points, first, total, channels=2, normalize=True, want_pcm=False):
        """gs_note_mix_curves (include/gansynth_hip.h): the notes of `table` -- host rows (onset, hold, release, row, gain, curve) -- mixed
        from the rows of waves [rows, L] fp32 under the piecewise-linear gain curves `points` / `first` (note_mix_curves_table).
        -> what note_mix returns with channels == 1 and what note_mix_stereo returns with channels == 2."""
        if channels not in (1, 2):
            raise ValueError(f"note_mix_curves: channels must be 1 or 2 (got {channels!r})")
        if waves.dim() != 2 or waves.dtype != torch.float32:
            raise ValueError(f"note_mix_curves: waves must be [rows, L] fp32 (got {tuple(waves.shape)} {waves.dtype})")
        rows, length = int(waves.shape[0]), int(waves.shape[1])
        total = int(total)
        arr, pts, firsts = note_mix_curves_table(table, points, first, rows, length, total)
        if waves.stride(1) != 1 or (rows > 1 and waves.stride(0) < length):
            waves = waves.contiguous()
        notes, pts_dev, first_dev = (torch.frombuffer(bytearray(bytes(a)), dtype=torch.uint8).to(waves.device) for a in (arr, pts, firsts))
        stride = (total + 3) // 4 * 4
        out = torch.empty((total,) if channels == 1 else (2, stride), dtype=torch.float32, device=waves.device)
        pcm = torch.empty((total,) if channels == 1 else (total, 2), dtype=torch.int16, device=waves.device) if want_pcm else None
        peak = torch.empty((1,), dtype=torch.float32, device=waves.device)
        ws = _ws(self.lib.gs_note_mix_curves_workspace_bytes(total), waves.device)
        _lib.check(self.lib.gs_note_mix_curves(waves.data_ptr(), rows, length, int(waves.stride(0)) if rows > 1 else length, notes.data_ptr(), len(arr),
                                               pts_dev.data_ptr(), len(pts), first_dev.data_ptr(), len(firsts) - 1, channels, total,
                                               1 if normalize else 0, out.data_ptr(), stride, None if pcm is None else pcm.data_ptr(),
                                               peak.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "gs_note_mix_curves")
        return (out if channels == 1 else out[:, :total]), pcm, peak

    def note_warp_table_dev(self, device):
        """gs_note_warp's coefficient table on `device`, built on the host and uploaded once per device."""
        device = torch.device(device)
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._warp_table:
            host = np.empty(self.lib.gs_note_warp_table_bytes() // 4, dtype=np.float32)
            _lib.check(self.lib.gs_note_warp_table(host.ctypes.data), "gs_note_warp_table")
            self._warp_table[key] = torch.from_numpy(host).to(device)
        return self._warp_table[key]

    def note_warp(self, waves, warp_notes, points, first):
        """gs_note_warp (include/gansynth_hip.h): for every row (src_row, dst_row, onset, count, curve) of `warp_notes`, the first `count`
        samples of waves[dst_row] become waves[src_row] played at the rate of its curve (`points` / `first`: note_warp_table), IN
        PLACE; nothing else is written.  waves: [rows, L] fp32 on the device with contiguous rows.  -> waves."""
        if waves.dim() != 2 or waves.dtype != torch.float32 or not waves.is_cuda:
            raise ValueError(f"note_warp: waves must be [rows, L] fp32 on the HIP device (got {tuple(waves.shape)} {waves.dtype} on {waves.device})")
        rows, length = int(waves.shape[0]), int(waves.shape[1])
        if waves.stride(1) != 1 or (rows > 1 and waves.stride(0) < length):
            raise ValueError(f"note_warp: the rows of waves must be contiguous and apart (strides {tuple(waves.stride())}): it works in place")
        arr, pts, firsts = note_warp_table(warp_notes, points, first, rows, length)
        if len(arr) > 65535:
            raise ValueError(f"note_warp: {len(arr)} notes are more than the 65535 of one call")
        table = self.note_warp_table_dev(waves.device)
        notes, pts_dev, first_dev = (torch.frombuffer(bytearray(bytes(a)), dtype=torch.uint8).to(waves.device) for a in (arr, pts, firsts))
        _lib.check(self.lib.gs_note_warp(waves.data_ptr(), rows, length, int(waves.stride(0)) if rows > 1 else length, notes.data_ptr(), len(arr),
                                         pts_dev.data_ptr(), first_dev.data_ptr(), len(firsts) - 1, len(pts), table.data_ptr(), _stream()),
                   "gs_note_warp")
        self.note_warps += 1
        return waves

    @staticmethod
    def _sustain_waves(what, waves):
        if waves.dim() != 2 or waves.dtype != torch.float32 or not waves.is_cuda:
            raise ValueError(f"{what}: waves must be [rows, L] fp32 on the HIP device (got {tuple(waves.shape)} {waves.dtype} on {waves.device})")
        rows, length = int(waves.shape[0]), int(waves.shape[1])
        if waves.stride(1) != 1 or (rows > 1 and waves.stride(0) < length):
            raise ValueError(f"{what}: the rows of waves must be contiguous and apart (strides {tuple(waves.stride())})")
        return rows, length, int(waves.stride(0)) if rows > 1 else length

    def loop_search(self, waves, rows_of_notes, plan):
        """gs_loop_search (include/gansynth_hip.h): for every row of `rows_of_notes` the normalised correlation of waves[row][a : a + W]
        with waves[row][a + m : a + m + W] for every lag m in [m_min, m_max]; `plan` = (a, m_min, m_max, W) or notes.sustain_plan's
        (a, m_min, m_max, W, X).  waves: [rows, L] fp32 on the device with contiguous rows; only read.
        -> scores [len(rows_of_notes), m_max - m_min + 1] fp32 on the device (notes.pick_loop picks from them on the host)."""
        rows, length, stride = self._sustain_waves("loop_search", waves)
        a, m_min, m_max, window = (plan[i] for i in range(4))
        n_lags = m_max - m_min + 1 if all(isinstance(v, (int, np.integer)) for v in (m_min, m_max)) else 1
        arr = loop_search_table([(row, a, m_min, m_max, window) for row in rows_of_notes], rows, length, n_lags)
        if len(arr) > 65535:
            raise ValueError(f"loop_search: {len(arr)} notes are more than the 65535 of one call")
        notes = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(waves.device)
        scores = torch.empty((len(arr), n_lags), dtype=torch.float32, device=waves.device)
        _lib.check(self.lib.gs_loop_search(waves.data_ptr(), rows, length, stride, notes.data_ptr(), len(arr), scores.data_ptr(), n_lags,
                                           _stream()), "gs_loop_search")
        self.loop_searches += 1
        return scores

    def note_sustain(self, waves, jobs):
        """gs_note_sustain (include/gansynth_hip.h): for every row (src_row, dst_row, offset, count, a, m, xfade) of `jobs`, the first
        `count` samples of waves[dst_row] become the samples offset .. offset + count of waves[src_row] looped over [a, a + m) with a
        crossfade of `xfade` samples, IN PLACE; nothing else is written.  waves: [rows, L] fp32 on the device with contiguous rows.
        -> waves."""
        rows, length, stride = self._sustain_waves("note_sustain", waves)
        arr = note_sustain_table(jobs, rows, length)
        if len(arr) > 65535:
            raise ValueError(f"note_sustain: {len(arr)} jobs are more than the 65535 of one call")
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(waves.device)
        _lib.check(self.lib.gs_note_sustain(waves.data_ptr(), rows, length, stride, table.data_ptr(), len(arr), _stream()), "gs_note_sustain")
        self.note_sustains += 1
        return waves

    def stereo_finish(self, x, normalize=True, want_pcm=False):
        """gs_stereo_finish (include/gansynth_hip.h): the second stage of note_mix_stereo on a clip x [2, n] fp32 that did not come from it
        (any row stride >= n), IN PLACE.  -> (x, pcm [n, 2] int16 or None, peak [1] fp32 = max |x| over both rows before any scaling);
        both rows are divided by peak when `normalize` and peak > 1."""
        if x.dim() != 2 or x.shape[0] != 2 or x.dtype != torch.float32 or not x.is_cuda or x.shape[1] == 0:
            raise ValueError(f"stereo_finish: x must be [2, n] fp32 on the HIP device (got {tuple(x.shape)} {x.dtype} on {x.device})")
        n = int(x.shape[1])
        if x.stride(1) != 1 or x.stride(0) < n:
            raise ValueError(f"stereo_finish: the rows of x must be contiguous and apart (strides {tuple(x.stride())}): it works in place")
        pcm = torch.empty((n, 2), dtype=torch.int16, device=x.device) if want_pcm else None
        peak = torch.empty((1,), dtype=torch.float32, device=x.device)
        ws = _ws(self.lib.gs_stereo_finish_workspace_bytes(n), x.device)
        _lib.check(self.lib.gs_stereo_finish(x.data_ptr(), n, int(x.stride(0)), 1 if normalize else 0, None if pcm is None else pcm.data_ptr(),
                                             peak.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "gs_stereo_finish")
        return x, pcm, peak

    def bank_gather(self, pcm, class_of_row, order, first, batch, n_classes, want_waves=True):
        """gs_bank_gather (include/gansynth_hip.h): the batch order[first : first + batch] of the resident bank pcm [rows, L] int16.
        -> (waves [batch, L] fp32 = pcm * 2^-15, or None without `want_waves`; labels [batch, n_classes] fp32 one-hot of class_of_row)."""
        if pcm.dim() != 2 or pcm.dtype != torch.int16:
            raise ValueError(f"bank_gather: pcm must be [rows, L] int16 (got {tuple(pcm.shape)} {pcm.dtype})")
        rows, length = int(pcm.shape[0]), int(pcm.shape[1])
        for name, t, n in (("class_of_row", class_of_row, rows), ("order", order, None)):
            if t.dim() != 1 or t.dtype != torch.int32 or not t.is_contiguous() or (n is not None and t.numel() != n):
                raise ValueError(f"bank_gather: {name} must be a contiguous int32 vector{'' if n is None else f' of {n} rows'} "
                                 f"(got {tuple(t.shape)} {t.dtype})")
        for name, t in (("pcm", pcm), ("class_of_row", class_of_row), ("order", order)):
            if not t.is_cuda or t.device != pcm.device:
                raise ValueError(f"bank_gather: {name} is on {t.device}, not on the bank's HIP device")
        if pcm.stride(1) != 1 or (rows > 1 and pcm.stride(0) < length):
            raise ValueError(f"bank_gather: pcm rows must be contiguous (strides {tuple(pcm.stride())}); the bank is not copied per draw")
        first, batch, n_classes = int(first), int(batch), int(n_classes)
        if batch <= 0 or n_classes <= 0 or first < 0 or first + batch > order.numel():
            raise ValueError(f"bank_gather: batch {batch} at first {first} with {n_classes} classes does not fit an order of {order.numel()}")
        waves = torch.empty((batch, length), dtype=torch.float32, device=pcm.device) if want_waves else None
        labels = torch.empty((batch, n_classes), dtype=torch.float32, device=pcm.device)
        _lib.check(self.lib.gs_bank_gather(pcm.data_ptr(), rows, length, int(pcm.stride(0)) if rows > 1 else length, class_of_row.data_ptr(),
                                           order.data_ptr(), order.numel(), first, batch, n_classes,
                                           None if waves is None else waves.data_ptr(), labels.data_ptr(), _stream()), "gs_bank_gather")
        return waves, labels

    def resample_design(self, rate_in, rate_out, device):
        """The design of rate_in -> rate_out and its table on `device` (in gs_resample's layout), built and uploaded once per
        (rate_in, rate_out, device): -> (GsResample, table tensor)."""
        device = torch.device(device)
        key = (int(rate_in), int(rate_out), device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._resample:
            design = _lib.GsResample()
            _lib.check(self.lib.gs_resample_design(key[0], key[1], ctypes.byref(design)), "gs_resample_design")
            host = np.empty(self.lib.gs_resample_table_bytes(ctypes.byref(design), 1) // 4, dtype=np.float32)
            _lib.check(self.lib.gs_resample_table(ctypes.byref(design), 1, host.ctypes.data), "gs_resample_table")
            self._resample[key] = (design, torch.from_numpy(host).to(device))
        return self._resample[key]

    def resample(self, x, rate_in, rate_out, normalize=False, want_pcm=False):
        """gs_resample (include/gansynth_hip.h): the rows of x -- [rows, n] or [n] fp32 on the device, any row stride -- from rate_in to
        rate_out.  -> (out [rows, n_out] fp32, pcm [rows, n_out] int16 or None, peak [rows] fp32 = max |y| per row before any scaling);
        a row of out is divided by its peak when `normalize` and that peak > 1."""
        if x.dim() not in (1, 2) or x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError(f"resample: x must be [rows, n] or [n] fp32 on the HIP device (got {tuple(x.shape)} {x.dtype} on {x.device})")
        if x.dim() == 1:
            x = x[None]
        rows, n_in = int(x.shape[0]), int(x.shape[1])
        if x.stride(1) != 1 or (rows > 1 and x.stride(0) < n_in):
            x = x.contiguous()
        design, table = self.resample_design(rate_in, rate_out, x.device)
        n_out = int(self.lib.gs_resample_out_len(ctypes.byref(design), n_in))
        if n_out <= 0:
            _lib.check(n_out, "gs_resample_out_len")
        out = torch.empty((rows, n_out), dtype=torch.float32, device=x.device)
        pcm = torch.empty((rows, n_out), dtype=torch.int16, device=x.device) if want_pcm else None
        peak = torch.empty((rows,), dtype=torch.float32, device=x.device)
        ws = _ws(self.lib.gs_resample_workspace_bytes(ctypes.byref(design), rows, n_in), x.device)
        _lib.check(self.lib.gs_resample(ctypes.byref(design), table.data_ptr(), x.data_ptr(), rows, n_in, int(x.stride(0)) if rows > 1 else n_in,
                                        1 if normalize else 0, out.data_ptr(), None if pcm is None else pcm.data_ptr(), peak.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream()), "gs_resample")
        return out, pcm, peak

    def fft_convolve_spectrum(self, design, impulse):
        """The prepared spectrum of `impulse` ([ir_rows, m] fp32 on the device) for gs_fftconv: built by ONE gs_fftconv_prepare per impulse
        tensor (keyed by its storage, shape, strides and version; the tensor is held, so that its address cannot be reused) and kept for
        the last few."""
        key = (impulse.data_ptr(), tuple(impulse.shape), tuple(impulse.stride()), impulse._version, impulse.device.index)
        hit = self._fftconv.get(key)
        if hit is None:
            nbytes = self.lib.gs_fftconv_spectrum_bytes(ctypes.byref(design))
            spectrum = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=impulse.device)
            _lib.check(self.lib.gs_fftconv_prepare(ctypes.byref(design), impulse.data_ptr(), int(impulse.stride(0)) if impulse.shape[0] > 1 else
                                                   int(impulse.shape[1]), spectrum.data_ptr(), spectrum.numel(), _stream()), "gs_fftconv_prepare")
            while len(self._fftconv) >= 8:
                self._fftconv.pop(next(iter(self._fftconv)))
            hit = self._fftconv[key] = (impulse, spectrum)
            self.fftconv_prepares += 1
        return hit[1]

    def fft_convolve(self, x, impulse, dry, wet, normalize=True, want_pcm=False):
        """gs_fftconv (include/gansynth_hip.h): y = dry * x + wet * (impulse convolved with x), row by row.  x: [n] or [rows, n] fp32 on the
        device, rows 1 or 2, any row stride; impulse: [m] or [ir_rows, m], ir_rows 1 (shared) or rows.  -> (out -- [n + m - 1] or
        [rows, n + m - 1] fp32, a view of rows that start on 16 bytes --, pcm [n + m - 1] or [n + m - 1, rows] int16 or None, peak [1]
        fp32 = max |y| over all rows before any scaling); every row is divided by that ONE peak when `normalize` and peak > 1."""
        rows, n, ir_rows, m = fft_convolve_shapes(x, impulse, dry, wet)
        for name, t in (("x", x), ("impulse", impulse)):
            if not t.is_cuda:
                raise ValueError(f"fft_convolve: {name} must be on the HIP device (it is on {t.device})")
        if impulse.device != x.device:
            raise ValueError(f"fft_convolve: impulse is on {impulse.device}, x on {x.device}")
        mono = x.dim() == 1
        x2 = x[None] if mono else x
        if x2.stride(1) != 1 or (rows > 1 and x2.stride(0) < n):
            x2 = x2.contiguous()
        h2 = impulse[None] if impulse.dim() == 1 else impulse
        if h2.stride(1) != 1 or (ir_rows > 1 and h2.stride(0) < m):
            raise ValueError(f"fft_convolve: the rows of impulse must be contiguous and apart (strides {tuple(impulse.stride())}): its spectrum is "
                             f"cached by its storage")
        design = _lib.GsFftConv()
        _lib.check(self.lib.gs_fftconv_design(n, m, rows, ir_rows, ctypes.byref(design)), "gs_fftconv_design")
        n_out = n + m - 1
        stride = (n_out + 3) // 4 * 4
        out = torch.empty((rows, stride), dtype=torch.float32, device=x.device)[:, :n_out]
        spectrum = self.fft_convolve_spectrum(design, h2)
        pcm = torch.empty((n_out,) if mono else (n_out, rows), dtype=torch.int16, device=x.device) if want_pcm else None
        peak = torch.empty((1,), dtype=torch.float32, device=x.device)
        ws = _ws(self.lib.gs_fftconv_workspace_bytes(ctypes.byref(design)), x.device)
        _lib.check(self.lib.gs_fftconv(ctypes.byref(design), spectrum.data_ptr(), spectrum.numel(), x2.data_ptr(), int(x2.stride(0)) if rows > 1 else n,
                                       float(dry), float(wet), 1 if normalize else 0, out.data_ptr(), int(out.stride(0)) if rows > 1 else n_out,
                                       None if pcm is None else pcm.data_ptr(), peak.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "gs_fftconv")
        return (out[0] if mono else out), pcm, peak

    def true_peak(self, x, want_envelope=True):
        """gs_true_peak (include/gansynth_hip.h): the 4x oversampled peak detector on x -- [n] or [rows, n] fp32 on the device, rows 1 or 2,
        any row stride.  -> (env [n] fp32 -- e[t] = the largest |value| of the reconstructed waveform of any row on [t, t + 1) -- or None,
        peak [1] fp32 = max e, the clip's true peak as a linear value).  The 1 -> 4 table is resample_design's, built once a device."""
        rows, n = true_peak_shapes(x)
        if not x.is_cuda:
            raise ValueError(f"true_peak: x must be on the HIP device (it is on {x.device})")
        x2 = x[None] if x.dim() == 1 else x
        if x2.stride(1) != 1 or (rows > 1 and x2.stride(0) < n):
            x2 = x2.contiguous()
        _, table = self.resample_design(1, _lib.TRUE_PEAK_OVERSAMPLE, x.device)
        env = torch.empty((n,), dtype=torch.float32, device=x.device) if want_envelope else None
        peak = torch.empty((1,), dtype=torch.float32, device=x.device)
        ws = _ws(self.lib.gs_true_peak_workspace_bytes(rows, n), x.device)
        _lib.check(self.lib.gs_true_peak(table.data_ptr(), x2.data_ptr(), rows, n, int(x2.stride(0)) if rows > 1 else n,
                                         None if env is None else env.data_ptr(), peak.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "gs_true_peak")
        return env, peak

    @staticmethod
    def _kmeans_rows(what, x, *others):
        """x as the k-means entries read it (unit column stride, rows at least d apart: a view with row slack is taken as it stands)."""
        if not x.is_cuda:
            raise ValueError(f"{what}: x must be on the HIP device (it is on {x.device})")
        for name, t in others:
            if t is not None and t.device != x.device:
                raise ValueError(f"{what}: {name} is on {t.device}, x on {x.device}")
        if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
            x = x.contiguous()
        return x, (int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1]))

    def kmeans_assign(self, x, centres, labels=None, want_dist=True, want_inertia=False):
        """gs_kmeans_assign (include/gansynth_hip.h): the nearest of centres [k, d] for every row of x [n, d] (fp32 on the device, any row stride)
        in the squared Euclidean distance, ties to the lowest index.  -> (labels [n] int32, dist [n] fp32 or None, changed [1] int32 or None,
        inertia [1] float64 or None: the sum of dist, accumulated in double).  `labels` given: it is read, overwritten and returned, and changed
        counts the rows whose label moved."""
        n, d, k = kmeans_assign_shapes(x, centres, labels)
        x2, ldx = self._kmeans_rows("kmeans_assign", x, ("centres", centres), ("labels", labels))
        centres = centres.contiguous()
        changed = torch.empty((1,), dtype=torch.int32, device=x.device) if labels is not None else None
        if labels is None:
            labels = torch.empty((n,), dtype=torch.int32, device=x.device)
        dist = torch.empty((n,), dtype=torch.float32, device=x.device) if want_dist else None
        inertia = torch.empty((1,), dtype=torch.float64, device=x.device) if want_inertia else None
        ws = _ws(self.lib.gs_kmeans_workspace_bytes(n, d, k), x.device)
        _lib.check(self.lib.gs_kmeans_assign(x2.data_ptr(), ldx, n, d, centres.data_ptr(), k, labels.data_ptr(), None if dist is None else dist.data_ptr(),
                                             None if changed is None else changed.data_ptr(), None if inertia is None else inertia.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream()), "gs_kmeans_assign")
        return labels, dist, changed, inertia

    def kmeans_inertia(self, x, centres, labels):
        """gs_kmeans_inertia (include/gansynth_hip.h): -> [1] float64, the sum over the rows of x [n, d] of the squared distance to the row of
        centres [k, d] that labels [n] (int32) names, every term and every sum in double, in a fixed order."""
        n, d, k = kmeans_inertia_shapes(x, centres, labels)
        x2, ldx = self._kmeans_rows("kmeans_inertia", x, ("centres", centres), ("labels", labels))
        centres = centres.contiguous()
        inertia = torch.empty((1,), dtype=torch.float64, device=x.device)
        ws = _ws(self.lib.gs_kmeans_workspace_bytes(n, d, k), x.device)
        _lib.check(self.lib.gs_kmeans_inertia(x2.data_ptr(), ldx, n, d, centres.data_ptr(), k, labels.data_ptr(), inertia.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _stream()), "gs_kmeans_inertia")
        return inertia

    def kmeans_update(self, x, labels, centres):
        """gs_kmeans_update (include/gansynth_hip.h): centres [k, d] (fp32, contiguous, on the device) receives, in place, the mean of the rows
        of x [n, d] of every label that has rows; an empty label's centre is left as it is.  -> counts [k] int32."""
        n, d, k = kmeans_update_shapes(x, labels, centres)
        x2, ldx = self._kmeans_rows("kmeans_update", x, ("labels", labels), ("centres", centres))
        counts = torch.empty((k,), dtype=torch.int32, device=x.device)
        ws = _ws(self.lib.gs_kmeans_workspace_bytes(n, d, k), x.device)
        _lib.check(self.lib.gs_kmeans_update(x2.data_ptr(), ldx, n, d, labels.data_ptr(), k, centres.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                             _stream()), "gs_kmeans_update")
        return counts

    def kmeans_mindist(self, x, centre, dist=None):
        """gs_kmeans_mindist (include/gansynth_hip.h), the k-means++ step: -> dist [n] fp32, |x_i - centre|^2 in a new vector, or, with `dist`
        given, the smaller of it and dist[i], in place."""
        n, d = kmeans_mindist_shapes(x, centre, dist)
        x2, ldx = self._kmeans_rows("kmeans_mindist", x, ("centre", centre), ("dist", dist))
        first = dist is None
        if first:
            dist = torch.empty((n,), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.gs_kmeans_mindist(x2.data_ptr(), ldx, n, d, centre.data_ptr(), dist.data_ptr(), 1 if first else 0, _stream()), "gs_kmeans_mindist")
        return dist

    def knn_kth(self, a, b, k, exclude_diagonal=False):
        """gs_knn_kth (include/gansynth_hip.h): -> [n, k] fp32, for every row of a [n, d] the k smallest squared distances to the rows of b [m, d]
        (fp32 on the device, any row stride), ascending; with `exclude_diagonal` row i of b is no candidate of row i of a (a set against itself).
        Where the candidates run out the rest is +inf."""
        n, m, d = knn_kth_shapes(a, b, k)
        a2, lda = self._kmeans_rows("knn_kth", a, ("b", b))
        b2, ldb = (a2, lda) if b is a else self._kmeans_rows("knn_kth", b)
        out = torch.empty((n, int(k)), dtype=torch.float32, device=a.device)
        ws = _ws(self.lib.gs_knn_workspace_bytes(n, m, d, int(k)), a.device)
        _lib.check(self.lib.gs_knn_kth(a2.data_ptr(), lda, n, b2.data_ptr(), ldb, m, d, int(k), 1 if exclude_diagonal else 0, out.data_ptr(), ws.data_ptr(),
                                       ws.numel(), _stream()), "gs_knn_kth")
        return out

    def knn_within(self, q, ref, radius2):
        """gs_knn_within (include/gansynth_hip.h): -> [n] int32, for every row of q [n, d] the number of rows j of ref [m, d] (fp32 on the device,
        any row stride) whose squared distance to it is at most radius2[j]."""
        n, m, d = knn_within_shapes(q, ref, radius2)
        q2, ldq = self._kmeans_rows("knn_within", q, ("ref", ref), ("radius2", radius2))
        r2, ldr = self._kmeans_rows("knn_within", ref)
        count = torch.empty((n,), dtype=torch.int32, device=q.device)
        ws = _ws(self.lib.gs_knn_workspace_bytes(n, m, d, 1), q.device)
        _lib.check(self.lib.gs_knn_within(q2.data_ptr(), ldq, n, r2.data_ptr(), ldr, m, d, radius2.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _stream()), "gs_knn_within")
        return count

    def kid_sums(self, x, y, xi=None, yi=None):
        """gs_kid_sums (include/gansynth_hip.h): -> [S, 3] float64 on the device, Sxx, Syy, Sxy of the cubic kernel k(a, b) = (a.b / d + 1)^3 over
        x [n, d] and y [m, d] (fp32 on the device, any row stride).  Without lists S = 1: the full sets.  With xi, yi ([S, size] integers, numpy or
        torch, anywhere): row r of subset s is x[xi[s, r]] / y[yi[s, r]]; the lists go to the device as int32."""
        n, m, d, subsets, size = kid_sums_shapes(x, y, xi, yi)
        x2, ldx = self._kmeans_rows("kid_sums", x, ("y", y))
        y2, ldy = (x2, ldx) if y is x else self._kmeans_rows("kid_sums", y)
        lists = [None, None]
        if subsets:
            lists = [(t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t).astype(np.int32))).to(device=x.device, dtype=torch.int32).contiguous()
                     for t in (xi, yi)]
        out = torch.empty((max(subsets, 1), 3), dtype=torch.float64, device=x.device)
        ws = _ws(self.lib.gs_kid_workspace_bytes(n, m, d, subsets, size), x.device)
        _lib.check(self.lib.gs_kid_sums(x2.data_ptr(), ldx, n, y2.data_ptr(), ldy, m, d, lists[0].data_ptr() if subsets else None,
                                        lists[1].data_ptr() if subsets else None, subsets, size, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "gs_kid_sums")
        return out

    def yin_difference(self, x, window, lags, hop):
        """gs_yin_difference (include/gansynth_hip.h): -> (d [rows, frames, lags] fp32, power [rows, frames] fp32) of x [rows, n] (fp32 on the
        device, any row stride): YIN's difference function in the direct form and the frame power."""
        rows, n, frames = yin_difference_shapes(x, window, lags, hop)
        x2, ldx = self._kmeans_rows("yin_difference", x)
        d = torch.empty((rows, frames, int(lags)), dtype=torch.float32, device=x.device)
        power = torch.empty((rows, frames), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.gs_yin_difference(x2.data_ptr(), ldx, rows, n, int(window), int(lags), int(hop), d.data_ptr(), power.data_ptr(), _stream()),
                   "gs_yin_difference")
        return d, power

    def yin_pick(self, d, tau_min, threshold):
        """gs_yin_pick (include/gansynth_hip.h): -> (lag [rows, frames] int32, period and aperiodicity [rows, frames] float64) from
        d [rows, frames, lags] (fp32, contiguous, on the device): cumulative-mean normalisation, pick and parabola in float64."""
        rows, frames, lags = yin_pick_shapes(d, tau_min, threshold)
        if not d.is_cuda:
            raise ValueError(f"yin_pick: d must be on the HIP device (it is on {d.device})")
        lag = torch.empty((rows, frames), dtype=torch.int32, device=d.device)
        period = torch.empty((rows, frames), dtype=torch.float64, device=d.device)
        aper = torch.empty((rows, frames), dtype=torch.float64, device=d.device)
        _lib.check(self.lib.gs_yin_pick(d.data_ptr(), rows, frames, lags, int(tau_min), float(threshold), lag.data_ptr(), period.data_ptr(), aper.data_ptr(),
                                        _stream()), "gs_yin_pick")
        return lag, period, aper

    def yin_track(self, x, window, lags, hop, tau_min, threshold):
        """gs_yin_track (include/gansynth_hip.h): one launch, -> (lag int32, period float64, aperiodicity float64, power fp32), each
        [rows, frames], of x [rows, n] (fp32 on the device, any row stride); bit for bit yin_pick(yin_difference(x))."""
        rows, n, frames = yin_track_shapes(x, window, lags, hop, tau_min, threshold)
        x2, ldx = self._kmeans_rows("yin_track", x)
        lag = torch.empty((rows, frames), dtype=torch.int32, device=x.device)
        period = torch.empty((rows, frames), dtype=torch.float64, device=x.device)
        aper = torch.empty((rows, frames), dtype=torch.float64, device=x.device)
        power = torch.empty((rows, frames), dtype=torch.float32, device=x.device)
        _lib.check(self.lib.gs_yin_track(x2.data_ptr(), ldx, rows, n, int(window), int(lags), int(hop), int(tau_min), float(threshold), lag.data_ptr(),
                                         period.data_ptr(), aper.data_ptr(), power.data_ptr(), _stream()), "gs_yin_track")
        return lag, period, aper, power

    @staticmethod
    def _swd_device(what, first, *others):
        if not first[1].is_cuda:
            raise ValueError(f"{what}: {first[0]} must be on the HIP device (it is on {first[1].device})")
        for name, t in others:
            if t.device != first[1].device:
                raise ValueError(f"{what}: {name} is on {t.device}, {first[0]} on {first[1].device}")

    def swd_pyramid(self, images):
        """gs_swd_pyramid (include/gansynth_hip.h): the Laplacian pyramid of images [b, 2, h, w] (fp32 or bf16 on the device; made channels-last
        when they are not) -> a list of its L levels, finest first, as fp32 [b, h >> l, w >> l, 2] views of one buffer."""
        b, h, w, levels = swd_pyramid_shapes(images)
        self._swd_device("swd_pyramid", ("images", images))
        x = _act(images)
        sizes = [b * (h >> l) * (w >> l) * 2 for l in range(levels)]
        lap = torch.empty((sum(sizes),), dtype=torch.float32, device=x.device)
        ws = _ws(self.lib.gs_swd_workspace_bytes(_lib.SWD_STAGE_PYRAMID, b, h, w), x.device)
        _lib.check(self.lib.gs_swd_pyramid(x.data_ptr(), _dt(x), b, h, w, lap.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "gs_swd_pyramid")
        out, at = [], 0
        for l, size in enumerate(sizes):
            out.append(lap[at:at + size].view(b, h >> l, w >> l, 2))
            at += size
        return out

    def swd_patches(self, level, ys, xs, desc, row_offset=0):
        """gs_swd_patches (include/gansynth_hip.h): the 128 7 x 7 patches an image of level [b, h, w, 2] at the corners ys, xs (int32 [b * 128] on
        the device) into the rows row_offset .. of desc [rows, 98], in place.  -> desc."""
        b, h, w = swd_patches_shapes(level, ys, xs, desc, row_offset)
        self._swd_device("swd_patches", ("level", level), ("ys", ys), ("xs", xs), ("desc", desc))
        _lib.check(self.lib.gs_swd_patches(level.data_ptr(), b, h, w, ys.data_ptr(), xs.data_ptr(), desc.data_ptr(), int(desc.shape[0]), int(row_offset),
                                           _stream()), "gs_swd_patches")
        return desc

    def swd_moments(self, desc):
        """gs_swd_moments (include/gansynth_hip.h): -> float64 [8]: the sum, the sum of squares, the mean and the population standard deviation
        of channel 0 (columns 0 .. 48 of desc [rows, 98]), then of channel 1."""
        rows = swd_desc_shapes("swd_moments", desc)
        self._swd_device("swd_moments", ("desc", desc))
        out = torch.empty((8,), dtype=torch.float64, device=desc.device)
        ws = _ws(self.lib.gs_swd_workspace_bytes(_lib.SWD_STAGE_MOMENTS, rows, 0, 0), desc.device)
        _lib.check(self.lib.gs_swd_moments(desc.data_ptr(), rows, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "gs_swd_moments")
        return out

    def swd_project(self, desc, moments, dirs):
        """gs_swd_project (include/gansynth_hip.h): desc [n, 98] normalised by `moments` (swd_moments's result) times dirs [98, ndir] -> fp32
        [ndir, n]: every direction's n values are contiguous."""
        n, ndir = swd_project_shapes(desc, moments, dirs)
        self._swd_device("swd_project", ("desc", desc), ("moments", moments), ("dirs", dirs))
        out = torch.empty((ndir, n), dtype=torch.float32, device=desc.device)
        _lib.check(self.lib.gs_swd_project(desc.data_ptr(), n, moments.data_ptr(), dirs.data_ptr(), ndir, out.data_ptr(), _stream()), "gs_swd_project")
        return out

    def swd_sort(self, data):
        """gs_swd_sort (include/gansynth_hip.h): every row of data [rows, n] (fp32, contiguous, on the device) ascending, in place.  -> data."""
        rows, n = swd_rows_shapes("swd_sort", "data", data)
        self._swd_device("swd_sort", ("data", data))
        ws = _ws(self.lib.gs_swd_workspace_bytes(_lib.SWD_STAGE_SORT, rows, n, 0), data.device)
        _lib.check(self.lib.gs_swd_sort(data.data_ptr(), rows, n, ws.data_ptr(), ws.numel(), _stream()), "gs_swd_sort")
        return data

    def swd_l1(self, a, b):
        """gs_swd_l1 (include/gansynth_hip.h): -> float64 [1], the sum of |a - b| over two [rows, n] buffers, in double and in a fixed order."""
        rows, n = swd_rows_shapes("swd_l1", "a", a)
        if (rows, n) != swd_rows_shapes("swd_l1", "b", b):
            raise ValueError(f"swd_l1: a and b differ in shape ({tuple(a.shape)} and {tuple(b.shape)})")
        self._swd_device("swd_l1", ("a", a), ("b", b))
        out = torch.empty((1,), dtype=torch.float64, device=a.device)
        ws = _ws(self.lib.gs_swd_workspace_bytes(_lib.SWD_STAGE_L1, rows, n, 0), a.device)
        _lib.check(self.lib.gs_swd_l1(a.data_ptr(), b.data_ptr(), rows, n, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "gs_swd_l1")
        return out

    def limit(self, x, pre_gain, ceiling, lookahead, want_pcm=False, envelope=None):
        """gs_limit (include/gansynth_hip.h): the look-ahead limiter on x -- [n] or [rows, n] fp32 on the device, rows 1 or 2, any row
        stride --: x times pre_gain, then ONE gain per sample for all rows that keeps every |sample| at or below ceiling, from the sliding
        minimum and mean over `lookahead` samples.  -> (out -- [n] or [rows, n] fp32, a new tensor whose rows start on 16 bytes --, pcm [n] or
        [n, rows] int16 or None, peak [1] fp32 = max |out|, min_gain [1] fp32 = the smallest gain applied).  `envelope` ([n] fp32 on the device,
        true_peak's of the same x): gs_limit_env -- the gain also keeps pre_gain * envelope at or below ceiling, i.e. the reconstructed waveform."""
        rows, n = limit_shapes(x, pre_gain, ceiling, lookahead)
        if not x.is_cuda:
            raise ValueError(f"limit: x must be on the HIP device (it is on {x.device})")
        if envelope is not None:
            envelope_shape(envelope, n)
            if envelope.device != x.device:
                raise ValueError(f"limit: envelope is on {envelope.device}, x on {x.device}")
            envelope = envelope.contiguous()
        mono = x.dim() == 1
        x2 = x[None] if mono else x
        if x2.stride(1) != 1 or (rows > 1 and x2.stride(0) < n):
            x2 = x2.contiguous()
        stride = (n + 3) // 4 * 4
        out = torch.empty((rows, stride), dtype=torch.float32, device=x.device)[:, :n]
        pcm = torch.empty((n,) if mono else (n, rows), dtype=torch.int16, device=x.device) if want_pcm else None
        peak = torch.empty((1,), dtype=torch.float32, device=x.device)
        min_gain = torch.empty((1,), dtype=torch.float32, device=x.device)
        ws = _ws(self.lib.gs_limit_workspace_bytes(rows, n), x.device)
        tail = (rows, n, int(x2.stride(0)) if rows > 1 else n, float(pre_gain), float(ceiling), int(lookahead), out.data_ptr(), stride,
                None if pcm is None else pcm.data_ptr(), peak.data_ptr(), min_gain.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        if envelope is None:
            _lib.check(self.lib.gs_limit(x2.data_ptr(), *tail), "gs_limit")
        else:
            _lib.check(self.lib.gs_limit_env(x2.data_ptr(), envelope.data_ptr(), *tail), "gs_limit_env")
        return (out[0] if mono else out), pcm, peak, min_gain

    def loudness_design(self, rate):
        """The K-weighting meter of `rate` (gs_loudness_design: host arithmetic), built once per rate: -> GsLoudness."""
        rate = int(rate)
        if rate not in self._loudness:
            design = _lib.GsLoudness()
            _lib.check(self.lib.gs_loudness_design(rate, ctypes.byref(design)), "gs_loudness_design")
            self._loudness[rate] = design
        return self._loudness[rate]

    def loudness_energy(self, x, rate):
        """gs_loudness (include/gansynth_hip.h): the BS.1770 K-weighted energy of every complete hop of floor(0.1 * rate + 0.5) samples of x
        -- [n] or [rows, n] fp32 on the device, rows 1 or 2, any row stride.  -> energy [rows, hops] fp32, hops = n // hop (possibly 0)."""
        rows, n = loudness_shapes(x, rate)
        if not x.is_cuda:
            raise ValueError(f"loudness_energy: x must be on the HIP device (it is on {x.device})")
        x2 = x[None] if x.dim() == 1 else x
        if x2.stride(1) != 1 or (rows > 1 and x2.stride(0) < n):
            x2 = x2.contiguous()
        design = self.loudness_design(rate)
        hops = int(self.lib.gs_loudness_hops(ctypes.byref(design), n))
        if hops < 0:
            _lib.check(hops, "gs_loudness_hops")
        energy = torch.empty((rows, hops), dtype=torch.float32, device=x.device)
        if hops == 0:   # no complete hop: nothing to measure (and an empty tensor has no address to hand over)
            return energy
        ws = _ws(self.lib.gs_loudness_workspace_bytes(ctypes.byref(design), rows, n), x.device)
        _lib.check(self.lib.gs_loudness(ctypes.byref(design), x2.data_ptr(), rows, n, int(x2.stride(0)) if rows > 1 else n, energy.data_ptr(),
                                        hops, ws.data_ptr(), ws.numel(), _stream()), "gs_loudness")
        return energy

    def account(self):
        """bench.py: `with K.account() as calls:` lists every kernel-layer call made inside as (method, argument dict, bytes read,
        bytes written) -- the algorithmic traffic of SURVEY.md 8(d): every tensor argument read once, every result written once
        (`out=` targets that are accumulated into: read and written).  Measurement only: the wrappers exist while the context does."""
        return _Accounting(self)

    def prof_enable(self, on):
        """on: False / True, or an int n > 1 for burst mode (every conv launch n times back to back inside its event pair)."""
        self.lib.gs_prof_enable(int(on))

    def prof_roofline(self, peak_tflops, peak_gbps):
        """(algorithmic bytes, roofline ms, HBM-bound part of it) of the recorded launches; call before prof_collect()."""
        b, r, rh = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        self.lib.gs_prof_roofline(float(peak_tflops), float(peak_gbps), ctypes.byref(b), ctypes.byref(r), ctypes.byref(rh))
        return b.value, r.value, rh.value

    def prof_records(self, max_records=8192):
        """[(ms, flops, bytes, (kind, N, Hb, Wb, IC, OC, a, b))] of the recorded launches; call before prof_collect()."""
        n = ctypes.c_int(0)
        ms = (ctypes.c_double * max_records)()
        fl = (ctypes.c_double * max_records)()
        by = (ctypes.c_double * max_records)()
        desc = (ctypes.c_int * (8 * max_records))()
        self.lib.gs_prof_records(max_records, ctypes.byref(n), ms, fl, by, desc)
        return [(ms[i], fl[i], by[i], tuple(desc[8 * i:8 * i + 8])) for i in range(n.value)]

    def prof_collect(self):
        n, ms, fl = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        self.lib.gs_prof_collect(ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl))
        return n.value, ms.value, fl.value


class _Accounting(object):
    SKIP = ("account", "prof_enable", "prof_roofline", "prof_records", "prof_collect", "register_param_buffer", "invalidate_weights", "early_flush_rule",
            "derived_slice", "defer_wgrad_reductions", "wgrad_slice_target_ok", "drop_deferred", "dense_nhwc_ok", "norm_bwd_bias_ok",
            "fwd_pnbwdbwd_is_fused", "bwd_data_pnbwd_is_fused", "conv2d_fwd_workspace", "resample_design", "loudness_design")

    def __init__(self, K):
        self.K, self.calls, self.depth, self.names = K, [], 0, []

    @staticmethod
    def _nbytes(obj):
        if isinstance(obj, torch.Tensor):
            return obj.numel() * obj.element_size()
        if isinstance(obj, (tuple, list)):
            return sum(_Accounting._nbytes(o) for o in obj)
        return 0

    def _wrap(self, name, fn):
        import inspect
        sig = inspect.signature(fn)

        def wrapper(*a, **kw):
            self.depth += 1
            try:
                out = fn(*a, **kw)
            finally:
                self.depth -= 1
            if self.depth == 0:   # (conv2d_fwd -> conv2d_fwd_bias_act ...: the outermost call is the one counted)
                try:
                    args = dict(sig.bind(*a, **kw).arguments)
                except TypeError:
                    args = {}
                read = sum(self._nbytes(v) for k, v in args.items() if k not in ("out", "bias_out"))
                if name == "bank_gather":   # a draw reads `batch` rows of the bank (none for labels alone), their classes and order entries
                    read = int(args["batch"]) * (8 + (2 * args["pcm"].shape[1] if args.get("want_waves", True) else 0))
                acc = sum(self._nbytes(args.get(k)) for k in ("out", "bias_out"))   # accumulated into: read + written
                written = self._nbytes(out) if acc == 0 or not isinstance(out, torch.Tensor) else 0
                meta = {k: (tuple(v.shape) if isinstance(v, torch.Tensor) else (tuple(v) if isinstance(v, (tuple, list, torch.Size)) else v))
                        for k, v in args.items()
                        if isinstance(v, (int, float, bool, torch.Tensor)) or v is None
                        or (isinstance(v, (tuple, list, torch.Size)) and all(isinstance(e, int) for e in v))}
                self.calls.append((name, meta, read + acc, written + acc))
            return out
        return wrapper

    def __enter__(self):
        for name in dir(type(self.K)):
            if name.startswith("_") or name in self.SKIP:
                continue
            fn = getattr(self.K, name)
            if callable(fn):
                setattr(self.K, name, self._wrap(name, fn))   # (instance attribute shadowing the method)
                self.names.append(name)
        return self.calls

    def __exit__(self, *exc):
        for name in self.names:
            try:
                delattr(self.K, name)
            except AttributeError:
                pass
        return False


class _StreamGuard(object):
    SKIP = _Accounting.SKIP + ("stream_guard", "refresh_weights", "flush_wgrad_reductions")

    hook = None   # class attribute: `hook(wrapper, name) -> wrapper` (debugging scripts only)

    def __init__(self, K):
        self.K, self.names = K, []

    @staticmethod
    def _mark(obj, stream):
        if isinstance(obj, torch.Tensor):
            if obj.is_cuda:
                obj.record_stream(stream)
        elif isinstance(obj, (tuple, list)):
            for o in obj:
                _StreamGuard._mark(o, stream)

    def _wrap(self, fn, name=""):
        mark = self._mark
        hook = self.hook   # (scripts/dbg_fork2.py: a recording wrapper around every call; None in production)

        def wrapper(*a, **kw):
            stream = torch.cuda.current_stream()
            for v in a:
                mark(v, stream)
            for v in kw.values():
                mark(v, stream)
            return fn(*a, **kw)
        return wrapper if hook is None else hook(wrapper, name)

    def __enter__(self):
        for name in dir(type(self.K)):
            if name.startswith("_") or name in self.SKIP or name in self.K.__dict__:
                continue
            fn = getattr(self.K, name)
            if callable(fn):
                setattr(self.K, name, self._wrap(fn, name))   # (instance attribute shadowing the method)
                self.names.append(name)
        self.K._guarding = True
        self.K._last_writer = {}
        return self

    def __exit__(self, *exc):
        self.K._guarding = False
        self.K._last_writer = {}
        for name in self.names:
            try:
                delattr(self.K, name)
            except AttributeError:
                pass
        return False


def completion_group(group_of, *targets):
    """The group (gradient bucket, in completion order) a deferred job runs in when it adds into several `targets` (a layer's weight
    gradient and, from the same launches, its bias gradient): the EARLIEST of their groups.  Buckets go on the wire in index order,
    bucket i right after the jobs of group i -- so a job must have run by the time the first bucket it touches is sent (the later
    ones are sent after it anyway).  (Also used by the CPU emulation of the tests.)"""
    tags = [group_of(t.data_ptr()) for t in targets if t is not None]
    tags = [t for t in tags if t is not None]
    return min(tags) if tags else None


def _match(t, ref):
    """Bring a gradient tensor to the dtype/layout of the activation it pairs with."""
    if t.dtype != ref.dtype:
        t = t.to(ref.dtype)
    if t.shape != ref.shape:
        t = t.expand(ref.shape)
    return _act(t)


_K = None


def get():
    """The process-wide kernel object (created on first use; raises without the library / a GPU)."""
    global _K
    if _K is None:
        _K = HipKernels()
    return _K


def set_backend(obj):
    """Test hook: install an object with the HipKernels interface (CPU emulation for autograd tests)."""
    global _K
    _K = obj
