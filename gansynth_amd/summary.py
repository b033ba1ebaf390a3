"""TensorBoard event files without TensorFlow (reference models.py:131-174, :327-367: the three SummarySaverHooks of train()).

`SummaryWriter(model_dir)` appends to `events.out.tfevents.<unix time>.<hostname>`: TFRecord framing around serialized `Event`
protos, both written by hand as dataset.py reads them by hand.  Images are 8-bit grayscale PNGs, audio is 16-bit PCM WAV, tags are
TF1's for max_outputs = 4 (`<name>/image/<i>`, `<name>/audio/<i>`, scalars `<name>`).

The float -> integer rules are tf.summary.image's and tf.summary.audio's (include/gansynth_hip.h states them).  Device tensors go
through the HIP kernels on the current stream and leave the device as bytes, through pinned buffers, followed by an event; host
tensors go through the numpy statement of the same two rules below, bit-identical to the kernels.  PNG / WAV encoding and the file
writes happen on one writer thread behind a bounded queue (what TF's EventFileWriter does), so the training loop waits for neither
the copy nor zlib; `flush()` drains the queue.

The field numbers are those of TensorFlow's event.proto / summary.proto as remembered; no TensorBoard has read these files yet.
"""
import os
import queue
import socket
import struct
import threading
import time
import zlib

import numpy as np
import torch

MAX_OUTPUTS = 4      # tf.summary.image / tf.summary.audio max_outputs (models.py:139, :153)
QUEUE_DEPTH = 16     # pending summary records (a GAN summary step enqueues three)
PNG_LEVEL = 6        # zlib's default


# ------------------------------------------------------------------------------------------------ checksums, framing
def _crc32c_table():
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1   # Castagnoli, reflected
        table.append(c)
    return table


_CRC_TABLE = _crc32c_table()


_CRC_NP = np.array(_CRC_TABLE, dtype=np.uint32)
_CRC_CHUNK = 1024     # bytes per lane of the vectorised form
_CRC_SHIFT = None     # four 256-entry tables: the register after _CRC_CHUNK zero bytes, by byte of the register before


def _crc32c_serial(data, crc):
    table = _CRC_TABLE
    for b in data:
        crc = table[(crc ^ b) & 0xFF] ^ (crc >> 8)
    return crc


def _crc_shift_tables():
    """The register update is linear over GF(2) in (register, byte): _CRC_CHUNK zero bytes map the register by a 32 x 32 bit matrix, kept
    as one table per register byte."""
    global _CRC_SHIFT
    if _CRC_SHIFT is None:
        basis = np.left_shift(np.uint32(1), np.arange(32, dtype=np.uint32))
        for _ in range(_CRC_CHUNK):
            basis = _CRC_NP[basis & 0xFF] ^ (basis >> 8)
        index = np.arange(256, dtype=np.uint32)
        tables = []
        for j in range(4):
            t = np.zeros(256, dtype=np.uint32)
            for i in range(8):
                t ^= np.where((index >> i) & 1, basis[8 * j + i], np.uint32(0)).astype(np.uint32)
            tables.append(t.tolist())
        _CRC_SHIFT = tables
    return _CRC_SHIFT


def crc32c(data):
    """CRC-32C (Castagnoli).  Table-driven, a byte at a time; a long message (a WAV, a PNG: ~100 KB each, 24 per GAN summary) runs
    _CRC_CHUNK-byte lanes side by side in numpy and joins them with the zero-byte shift of the register, so that the writer thread
    does not hold the interpreter for a byte loop over megabytes."""
    data = bytes(data)
    lanes = len(data) // _CRC_CHUNK
    if lanes < 8:
        return _crc32c_serial(data, 0xFFFFFFFF) ^ 0xFFFFFFFF
    head = len(data) - lanes * _CRC_CHUNK
    crc = _crc32c_serial(data[:head], 0xFFFFFFFF)
    columns = np.frombuffer(data, dtype=np.uint8, offset=head).reshape(lanes, _CRC_CHUNK).T.astype(np.uint32)
    raw = np.zeros(lanes, dtype=np.uint32)           # every lane from a zero register
    for column in columns:
        raw = _CRC_NP[(raw ^ column) & 0xFF] ^ (raw >> 8)
    t0, t1, t2, t3 = _crc_shift_tables()
    for r in raw.tolist():
        crc = t0[crc & 0xFF] ^ t1[(crc >> 8) & 0xFF] ^ t2[(crc >> 16) & 0xFF] ^ t3[crc >> 24] ^ r
    return crc ^ 0xFFFFFFFF


def masked_crc(data):
    crc = crc32c(data)
    return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def tfrecord(data):
    """One framed record: u64 length, u32 masked_crc(length bytes), data, u32 masked_crc(data), little-endian."""
    head = struct.pack("<Q", len(data))
    return b"".join((head, struct.pack("<I", masked_crc(head)), data, struct.pack("<I", masked_crc(data))))


# ------------------------------------------------------------------------------------------------ protobuf wire format
def _varint(n):
    n &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _int(field, value):
    return _varint(field << 3) + _varint(int(value))


def _bytes(field, data):
    return _varint(field << 3 | 2) + _varint(len(data)) + data


def _float(field, value):
    return _varint(field << 3 | 5) + struct.pack("<f", value)


def _double(field, value):
    return _varint(field << 3 | 1) + struct.pack("<d", value)


def event(wall_time, step=None, file_version=None, values=()):
    """Event{wall_time = 1, step = 2, file_version = 3, summary = 5{value = 1 (repeated)}}."""
    out = _double(1, wall_time)
    if step is not None:
        out += _int(2, step)
    if file_version is not None:
        out += _bytes(3, file_version.encode())
    if values:
        out += _bytes(5, b"".join(_bytes(1, v) for v in values))
    return out


def scalar_value(tag, value):
    """Summary.Value{tag = 1, simple_value = 2}."""
    return _bytes(1, tag.encode()) + _float(2, float(value))


def image_value(tag, height, width, png):
    """Summary.Value{tag = 1, image = 4{height = 1, width = 2, colorspace = 3 (1: grayscale), encoded_image_string = 4}}."""
    return _bytes(1, tag.encode()) + _bytes(4, _int(1, height) + _int(2, width) + _int(3, 1) + _bytes(4, png))


def audio_value(tag, sample_rate, frames, wav):
    """Summary.Value{tag = 1, audio = 6{sample_rate = 1, num_channels = 2, length_frames = 3, encoded_audio_string = 4, content_type = 5}}."""
    return _bytes(1, tag.encode()) + _bytes(6, _float(1, float(sample_rate)) + _int(2, 1) + _int(3, frames) + _bytes(4, wav) + _bytes(5, b"audio/wav"))


# ------------------------------------------------------------------------------------------------ encoders
def png_gray8(pixels, level=PNG_LEVEL):
    """uint8 [H, W] -> an 8-bit grayscale PNG (filter 0 on every row)."""
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    h, w = pixels.shape
    rows = np.zeros((h, w + 1), dtype=np.uint8)
    rows[:, 1:] = pixels

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    return b"".join((b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)),
                     chunk(b"IDAT", zlib.compress(rows.tobytes(), level)), chunk(b"IEND", b"")))


def wav_pcm16(samples, sample_rate):
    """int16 [L] -> RIFF/WAVE, 16-bit PCM, mono."""
    data = np.ascontiguousarray(samples, dtype="<i2").tobytes()
    rate = int(sample_rate)
    fmt = struct.pack("<HHIIHH", 1, 1, rate, rate * 2, 2, 16)
    return b"".join((b"RIFF", struct.pack("<I", 36 + len(data)), b"WAVE", b"fmt ", struct.pack("<I", len(fmt)), fmt,
                     b"data", struct.pack("<I", len(data)), data))


# ------------------------------------------------------------------------------------------------ the two rules on the host
def quantise_images_host(planes):
    """tf.summary.image's rule on float32 planes [..., H, W], each plane on its own: uint8 of the same shape.  Bit-identical to
    gs_summary_image_u8: fp32 throughout, the multiply and the add as two roundings."""
    x = np.ascontiguousarray(planes, dtype=np.float32)
    flat = x.reshape(-1, x.shape[-2] * x.shape[-1])
    out = np.empty(flat.shape, dtype=np.uint8)
    with np.errstate(all="ignore"):
        for plane, q in zip(flat, out):
            finite = np.isfinite(plane)
            q[:] = 255
            if not finite.any():
                continue
            v = plane[finite]
            lo, hi = v.min(), v.max()
            if lo < 0:
                m = max(abs(lo), abs(hi))
                scale = np.float32(0) if m < np.float32(1e-6) else np.float32(127) / m
                offset = np.float32(128)
            else:
                scale = np.float32(0) if hi < np.float32(1e-6) else np.float32(255) / hi
                offset = np.float32(0)
            q[finite] = np.trunc((v * scale).astype(np.float32) + offset).astype(np.uint8)
    return out.reshape(x.shape)


def quantise_audio_host(waveforms):
    """TF's FloatToInt16Sample on float32 samples: clamp(roundf(x * 32768), -32768, 32767), halves away from zero, NaN -> 0."""
    x = np.ascontiguousarray(waveforms, dtype=np.float32)
    with np.errstate(all="ignore"):
        y = x * np.float32(32768)            # exact: a power of two
        r = np.trunc(y)
        frac = y - r                         # exact; NaN for the infinities, which are integers already
        r = r + np.where(np.abs(frac) >= np.float32(0.5), np.copysign(np.float32(1), y), np.float32(0)).astype(np.float32)
        r = np.clip(r, np.float32(-32768), np.float32(32767))
        r = np.where(np.isnan(x), np.float32(0), r)
    return r.astype(np.int16)


# ------------------------------------------------------------------------------------------------ device -> host
class _Pending(object):
    """A quantised batch on its way to the host: `array()` waits for the copy (on the writer thread) and returns the numpy view."""

    def __init__(self, device_tensor):
        self.host = torch.empty(device_tensor.shape, dtype=device_tensor.dtype, pin_memory=True)
        self.host.copy_(device_tensor, non_blocking=True)
        self.done = torch.cuda.Event()
        self.done.record()

    def array(self):
        self.done.synchronize()
        return self.host.numpy()


class _Ready(object):
    def __init__(self, array):
        self._array = array

    def array(self):
        return self._array


def _image_planes(tensor):
    """[B, H, W] or [B, 2, H, W] -> quantised uint8 [n, C, H, W] of the first min(B, 4) items (pending for a device tensor)."""
    if tensor.dim() not in (3, 4) or (tensor.dim() == 4 and tensor.shape[1] not in (1, 2)):
        raise ValueError(f"summary images are [B, H, W] or [B, 2, H, W] (got {tuple(tensor.shape)})")
    if tensor.is_cuda:
        from . import kernels
        return _Pending(kernels.get().summary_image_u8(tensor.detach(), MAX_OUTPUTS))
    x = tensor.detach()[:MAX_OUTPUTS].float().numpy()
    if x.ndim == 3:
        x = x[:, None]
    return _Ready(quantise_images_host(x))


def _audio_rows(tensor):
    if tensor.dim() != 2:
        raise ValueError(f"summary audio is [B, L] (got {tuple(tensor.shape)})")
    if tensor.is_cuda:
        from . import kernels
        return _Pending(kernels.get().summary_audio_s16(tensor.detach(), MAX_OUTPUTS))
    return _Ready(quantise_audio_host(tensor.detach()[:MAX_OUTPUTS].float().numpy()))


# ------------------------------------------------------------------------------------------------ the writer
class SummaryWriter(object):
    """scalars / images / audio -> one Event record each, appended to the events file of `model_dir` by the writer thread.  The file
    (and the thread) appear with the first record handed over: a run that never reaches a summary step leaves nothing behind."""

    def __init__(self, model_dir, queue_depth=QUEUE_DEPTH, png_level=PNG_LEVEL):
        self.model_dir, self.queue_depth, self.png_level = model_dir, queue_depth, png_level
        self.path = None
        self._file = self._queue = self._thread = self._error = None
        self._closed = False

    def _open(self):
        os.makedirs(self.model_dir, exist_ok=True)
        now = time.time()
        self.path = os.path.join(self.model_dir, f"events.out.tfevents.{int(now):010d}.{socket.gethostname()}")
        self._file = open(self.path, "ab")
        self._file.write(tfrecord(event(now, file_version="brain.Event:2")))
        self._file.flush()
        self._queue = queue.Queue(maxsize=self.queue_depth)
        self._thread = threading.Thread(target=self._work, name="summary-writer", daemon=True)
        self._thread.start()

    # ---- the training loop's side
    def scalars(self, step, values):
        self._put(step, [("scalar", name, float(v)) for name, v in values.items()])

    def images(self, step, tensors):
        """{name: [B, H, W]}; or {(name of plane 0, name of plane 1): [B, 2, H, W]} -- both planes of channels-last images at once."""
        items = []
        for name, t in tensors.items():
            names = (name,) if isinstance(name, str) else tuple(name)
            if len(names) != (t.shape[1] if t.dim() == 4 else 1):
                raise ValueError(f"{names}: {len(names)} names for an image tensor of shape {tuple(t.shape)}")
            items.append(("image", names, _image_planes(t)))
        self._put(step, items)

    def audio(self, step, tensors, sample_rate):
        self._put(step, [("audio", name, _audio_rows(t), int(sample_rate)) for name, t in tensors.items()])

    def flush(self):
        """Everything handed over so far is in the file."""
        if self._thread is not None:
            self._queue.join()
            self._raise()
            self._file.flush()

    def close(self):
        self._closed = True
        if self._thread is not None:
            self._queue.put(None)
            self._thread.join()
            self._thread = None
            self._file.close()
        self._raise()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _put(self, step, items):
        self._raise()
        if self._closed:
            raise ValueError("SummaryWriter is closed")
        if self._thread is None:
            self._open()
        self._queue.put((int(step), time.time(), items))

    def _raise(self):
        if self._error is not None:
            error, self._error = self._error, None
            raise RuntimeError("the summary writer thread failed") from error

    # ---- the writer thread's side
    def _values(self, items):
        for item in items:
            kind, name = item[0], item[1]
            if kind == "scalar":
                yield scalar_value(name, item[2])
            elif kind == "image":
                planes = item[2].array()   # [n, C, H, W]
                for c, plane_name in enumerate(name):
                    for i in range(planes.shape[0]):
                        yield image_value(f"{plane_name}/image/{i}", planes.shape[2], planes.shape[3], png_gray8(planes[i, c], self.png_level))
            else:
                rows = item[2].array()     # [n, L]
                for i in range(rows.shape[0]):
                    yield audio_value(f"{name}/audio/{i}", item[3], rows.shape[1], wav_pcm16(rows[i], item[3]))

    def _work(self):
        while True:
            job = self._queue.get()
            try:
                if job is None:
                    return
                step, wall_time, items = job
                self._file.write(tfrecord(event(wall_time, step=step, values=list(self._values(items)))))
            except BaseException as e:   # noqa: BLE001 -- handed to the training thread (flush / the next record raises it); the record is lost
                self._error = e
            finally:
                self._queue.task_done()
