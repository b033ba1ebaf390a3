"""What the summary kernels and the event-file writer are held to (tests/test_summary_cpu.py, tests/test_summary_gpu.py).

The two float -> integer rules are restated here in numpy float32, plane by plane, the multiply and the add as separate float32
operations.  They are written from memory of TensorFlow 1.13 -- tf.summary.image's float branch in summary_image_op.cc, and
FloatToInt16Sample in wav_io.cc as tf.summary.audio uses it -- and TensorFlow cannot be installed next to this tree: THIS restatement,
not TensorFlow, is the definition gs_summary_image_u8 / gs_summary_audio_s16 and their host fallback are tested against, bit for bit.

  image, per image and per channel plane:  lo, hi = min, max over the FINITE values;
      lo < 0:  m = max(|lo|, |hi|), scale = 0 if m < 1e-6 else 127 / m, offset = 128
      else:    scale = 0 if hi < 1e-6 else 255 / hi, offset = 0
      finite v -> uint8(trunc(fl(fl(v * scale) + offset))), non-finite v -> 255 (a plane without a finite value: all 255)
  audio:  clamp(roundf(x * 32768), -32768, 32767), roundf rounding halves away from zero; NaN -> 0 (this tree's choice: TF's is undefined)

The readers below take an events file apart with code that is not under test: gansynth_amd.dataset's TFRecord / protobuf readers (the
input pipeline's), PIL for the PNGs, scipy.io.wavfile for the WAVs.
"""
import functools
import io
import math
import struct

import numpy as np

F32 = np.float32


def image_u8(plane):
    """One plane (any shape) of float32 values -> uint8 of the same shape."""
    plane = np.asarray(plane, dtype=F32)
    flat = plane.reshape(-1)
    finite = np.isfinite(flat)
    out = np.full(flat.shape, 255, dtype=np.uint8)
    if finite.any():
        lo, hi = F32(flat[finite].min()), F32(flat[finite].max())
        if lo < 0:
            m = max(abs(lo), abs(hi))
            scale, offset = (F32(0) if m < F32(1e-6) else F32(127) / F32(m)), F32(128)
        else:
            scale, offset = (F32(0) if hi < F32(1e-6) else F32(255) / F32(hi)), F32(0)
        with np.errstate(all="ignore"):
            t = np.multiply(flat, scale, dtype=F32)     # rounded to float32 ...
            r = np.add(t, offset, dtype=F32)            # ... before the add: two operations, two roundings
        out[finite] = np.trunc(r[finite]).astype(np.uint8)
    return out.reshape(plane.shape)


def images_u8(x):
    """[N, C, H, W] float32 -> uint8, every (image, channel) plane on its own."""
    x = np.asarray(x, dtype=F32)
    return np.stack([np.stack([image_u8(p) for p in img]) for img in x])


def audio_s16(x):
    """float32 samples (any shape) -> int16."""
    x = np.asarray(x, dtype=F32)
    out = np.zeros(x.shape, dtype=np.int16).reshape(-1)
    for i, v in enumerate(x.reshape(-1)):
        if math.isnan(v):
            continue
        y = float(F32(v) * F32(32768))      # exact in float32 (a power of two), or +-inf
        if math.isinf(y):
            r = y
        else:
            r = math.floor(abs(y) + 0.5) * (1.0 if y >= 0 else -1.0)   # halves away from zero; exact in float64
        out[i] = int(min(max(r, -32768.0), 32767.0))
    return out.reshape(x.shape)


# ---------------------------------------------------------------------------------------------------------------- readers
def crc32c(data):
    """CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) a bit at a time: slow and plain, for the small files of the tests."""
    crc = 0xFFFFFFFF
    for b in bytes(data):
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0x82F63B78 if crc & 1 else crc >> 1
    return crc ^ 0xFFFFFFFF


def masked_crc(data):
    crc = crc32c(data)
    return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def check_record_crcs(path):
    """Every record's two masked CRC-32C words against the bit-at-a-time form above.  Returns the number of records."""
    count = 0
    with open(path, "rb") as f:
        blob = f.read()
    pos = 0
    while pos < len(blob):
        head = blob[pos:pos + 8]
        (n,) = struct.unpack("<Q", head)
        (crc_head,) = struct.unpack("<I", blob[pos + 8:pos + 12])
        data = blob[pos + 12:pos + 12 + n]
        assert len(data) == n and len(blob) >= pos + 16 + n, "truncated record"
        (crc_data,) = struct.unpack("<I", blob[pos + 12 + n:pos + 16 + n])
        assert crc_head == masked_crc(head), f"record {count}: length CRC"
        assert crc_data == masked_crc(data), f"record {count}: data CRC"
        pos += 16 + n
        count += 1
    return count


def read_events(path):
    """[{wall_time, step, file_version, values: [{tag, simple_value | image: (h, w, colorspace, png) | audio: (rate, channels, frames,
    wav, content_type)}]}] of an events file."""
    from gansynth_amd.dataset import _fields, tfrecord_iterator
    events = []
    for record in tfrecord_iterator(path):
        ev = dict(wall_time=None, step=0, file_version=None, values=[])
        for num, wt, val in _fields(record):
            if num == 1 and wt == 1:
                (ev["wall_time"],) = struct.unpack("<d", bytes(val))
            elif num == 2 and wt == 0:
                ev["step"] = val
            elif num == 3 and wt == 2:
                ev["file_version"] = bytes(val).decode()
            elif num == 5 and wt == 2:
                for snum, swt, sval in _fields(val):
                    if snum == 1 and swt == 2:
                        ev["values"].append(_value(sval))
        events.append(ev)
    return events


def _value(buf):
    from gansynth_amd.dataset import _fields
    out = {}
    for num, wt, val in _fields(buf):
        if num == 1 and wt == 2:
            out["tag"] = bytes(val).decode()
        elif num == 2 and wt == 5:
            (out["simple_value"],) = struct.unpack("<f", bytes(val))
        elif num == 4 and wt == 2:
            f = {n: v for n, _, v in _fields(val)}
            out["image"] = (f[1], f[2], f[3], bytes(f[4]))
        elif num == 6 and wt == 2:
            f = {n: v for n, _, v in _fields(val)}
            (rate,) = struct.unpack("<f", bytes(f[1]))
            out["audio"] = (rate, f[2], f[3], bytes(f[4]), bytes(f[5]).decode())
    return out


def tags(events, step=None):
    return [v["tag"] for ev in events if step is None or ev["step"] == step for v in ev["values"]]


def find(events, tag, step):
    hits = [v for ev in events if ev["step"] == step for v in ev["values"] if v["tag"] == tag]
    assert len(hits) == 1, (tag, step, len(hits))
    return hits[0]


def decode_png(value):
    """Summary.Value with an image -> uint8 [H, W] (PIL), after checking the proto's height / width / colorspace against the file."""
    from PIL import Image
    h, w, colorspace, png = value["image"]
    img = Image.open(io.BytesIO(png))
    assert img.mode == "L" and img.size == (w, h) and colorspace == 1
    return np.asarray(img, dtype=np.uint8)


def decode_wav(value):
    """Summary.Value with audio -> (rate from the WAV header, int16 [L]) (scipy), after checking the proto's fields against the file."""
    from scipy.io import wavfile
    rate, channels, frames, wav, content_type = value["audio"]
    file_rate, data = wavfile.read(io.BytesIO(wav))
    assert data.dtype == np.int16 and data.ndim == 1 and channels == 1 and frames == data.shape[0]
    assert content_type == "audio/wav" and float(file_rate) == rate
    return file_rate, data


# ------------------------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def image_cases():
    """{name: float32 [N, P, C] interleaved} -- the kernel's input layout; [N, C, P] planes are x.transpose(0, 2, 1)."""
    rng = np.random.default_rng(20)
    cases = {}
    for c in (1, 2):
        cases[f"odd_tail_c{c}"] = rng.standard_normal((3, 5 * 37, c)).astype(F32)
        big = rng.uniform(-0.5, 0.5, (1, 128 * 1024, c)).astype(F32)
        big[0, -7, :] = -3.0      # the minimum in the last slab ...
        big[0, 5, :] = 2.0        # ... the maximum in the first: the fold crosses slabs
        cases[f"cross_slab_c{c}"] = big
        p = 2 * 2048 + 36         # three slabs, the last one short
        mixed = rng.standard_normal((1, p, c)).astype(F32)
        nonneg = np.abs(rng.standard_normal((1, p, c))).astype(F32)
        tiny = rng.uniform(-9e-7, 9e-7, (1, p, c)).astype(F32)
        tiny_pos = rng.uniform(0, 9e-7, (1, p, c)).astype(F32)
        planted = rng.standard_normal((1, p, c)).astype(F32)
        planted[0, 0, :], planted[0, -1, :], planted[0, 2048 + 1000, :] = np.nan, np.inf, -np.inf
        planted_pos = np.abs(planted)
        planted_pos[0, 0, :] = np.nan
        nothing = np.full((1, p, c), np.nan, dtype=F32)
        nothing[0, 1::3, :], nothing[0, 2::3, :] = np.inf, -np.inf
        cases[f"branches_c{c}"] = np.concatenate([mixed, nonneg, tiny, tiny_pos, planted, planted_pos, nothing])
    return cases


def to_bf16(x):
    """float32 array rounded to bfloat16 (nearest even, torch's conversion) and widened again."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).bfloat16().float().numpy()


@functools.lru_cache(maxsize=None)
def image_reference(name, bf16=False):
    """uint8 [N, C, P]: the restatement on image_cases()[name] (`bf16`: on the inputs rounded to bfloat16), computed once."""
    x = image_cases()[name]
    x = to_bf16(x) if bf16 else x
    return images_u8(x.transpose(0, 2, 1)[..., None])[..., 0]


@functools.lru_cache(maxsize=None)
def audio_case():
    """float32 [2, 1003]: random samples around the clamp, then the values the rule turns on."""
    rng = np.random.default_rng(21)
    x = rng.uniform(-1.2, 1.2, (2, 1003)).astype(F32)
    ks = np.array([0, 1, 2, 3, 100, 101, 32766, 32767, -1, -2, -3, -4, -101, -102, -32768, -32769], dtype=np.float64)
    special = np.concatenate([[1.0, -1.0, 1.5, -1.5, np.nan, np.inf, -np.inf, 0.0, -0.0, 0.49999997 / 32768], (ks + 0.5) / 32768.0])
    x[0, :special.size] = special.astype(F32)
    x[1, -special.size:] = special.astype(F32)[::-1]
    return x
