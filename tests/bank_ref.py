"""What gs_bank_gather and the resident feed are held to (include/gansynth_hip.h, DESIGN.md "Resident notes"): the gather in numpy,
and the small writers of record files and WAVs the bank tests share.  Nothing here imports gansynth_amd.bank."""
import json
import os
import struct
import wave

import numpy as np


def gather(pcm, class_of_row, order, first, batch, n_classes, want_waves=True):
    """pcm int16 [rows, length], class_of_row int32 [rows], order int32 [n] -> (waves [batch, length] fp32 or None, labels
    [batch, n_classes] fp32).  A row outside [0, rows) is silence with an all-zero label; a class outside [0, n_classes) an all-zero label."""
    pcm, class_of_row, order = np.asarray(pcm), np.asarray(class_of_row), np.asarray(order)
    rows, length = pcm.shape
    assert pcm.dtype == np.int16 and 0 <= first and first + batch <= len(order)
    waves = np.zeros((batch, length), dtype=np.float32) if want_waves else None
    labels = np.zeros((batch, n_classes), dtype=np.float32)
    for b in range(batch):
        r = int(order[first + b])
        if not 0 <= r < rows:
            continue
        if want_waves:
            waves[b] = pcm[r].astype(np.float32) * np.float32(2.0 ** -15)   # exact: |pcm| <= 2^15 has 16 significant bits at most
        c = int(class_of_row[r])
        if 0 <= c < n_classes:
            labels[b, c] = 1.0
    return waves, labels


# ---------------------------------------------------------------------------------------------------- record files and WAVs
def _varint(n):
    out = b""
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out += bytes([b | 0x80])
        else:
            return out + bytes([b])


def _ld(field, payload):   # length-delimited protobuf field
    return _varint((field << 3) | 2) + _varint(len(payload)) + payload


def example(path, pitch, source):
    """tf.train.Example{features{feature{"path": bytes_list, "pitch": int64_list, "source": int64_list}}}, written by hand."""
    def int_feature(v):
        return _ld(3, _varint((1 << 3) | 0) + _varint(v & ((1 << 64) - 1)))
    feats = b""
    for name, feature in (("path", _ld(1, _ld(1, path.encode()))), ("pitch", int_feature(pitch)), ("source", int_feature(source))):
        feats += _ld(1, _ld(1, name.encode()) + _ld(2, feature))
    return _ld(1, feats)


def write_tfrecord(filename, records):
    """records: (path, pitch, source) triples."""
    with open(filename, "wb") as f:
        for path, pitch, source in records:
            ex = example(path, pitch, source)
            f.write(struct.pack("<Q", len(ex)) + b"\0\0\0\0" + ex + b"\0\0\0\0")


def write_wav(path, samples, channels=1):
    """samples: int16 values, interleaved when channels > 1."""
    with wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.asarray(samples, dtype="<i2").tobytes())


def write_notes(directory, count, samples, pitches, sources, seed=0, split=None):
    """`count` mono WAVs of `samples` random int16 values each under `directory`; sample 0 of note i is i + 1, so a decoded row names its
    file.  Their records go into one tfrecord, or two when `split` is a position.  -> (record files, [(path, pitch, source, pcm)])."""
    rng = np.random.default_rng(seed)
    notes = []
    for i in range(count):
        pcm = rng.integers(-32768, 32768, size=samples).astype(np.int16)
        pcm[0] = i + 1
        path = os.path.join(str(directory), f"note{i:03d}.wav")
        write_wav(path, pcm)
        notes.append((path, int(pitches[i % len(pitches)]), int(sources[i % len(sources)]), pcm))
    cuts = [0, count] if split is None else [0, split, count]
    files = []
    for k in range(len(cuts) - 1):
        files.append(os.path.join(str(directory), f"notes_{k}.tfrecord"))
        write_tfrecord(files[-1], [n[:3] for n in notes[cuts[k]:cuts[k + 1]]])
    return files, notes


def write_examples_json(directory, notes):
    """NSynth's layout: <directory>/examples.json next to <directory>/audio/<name>.wav.  notes: {name: (pitch, source, samples, channels)}."""
    os.makedirs(os.path.join(str(directory), "audio"), exist_ok=True)
    index = {}
    for name, (pitch, source, samples, channels) in notes.items():
        write_wav(os.path.join(str(directory), "audio", name + ".wav"), samples, channels)
        index[name] = {"pitch": pitch, "instrument_source": source}
    path = os.path.join(str(directory), "examples.json")
    with open(path, "w") as f:
        json.dump(index, f)
    return path
