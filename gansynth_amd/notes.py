"""Note sequences: the score reader and the schedule of GANSynth.synthesize (host, pure Python; DESIGN.md "Note sequences").

The reference has no renderer: the rules here are this project's own.  A `Note` is (pitch, velocity, start, end) -- a MIDI number, 1..127,
and seconds with 0 <= start < end.  `read_notes` reads a JSON list or a Standard MIDI File (format 0 or 1); `schedule` turns notes into
the sample-exact table that kernels.HipKernels.note_mix mixes; `schedule_latents` gives every note its latent by spherical
interpolation between anchors drawn from a generator of their own (the global RNG, and with it a training run's stream, does not move).
"""
import collections
import json
import math
import os
import struct

import numpy as np
import torch

Note = collections.namedtuple("Note", ["pitch", "velocity", "start", "end"])

DEFAULT_TEMPO = 500000   # microseconds per quarter note until a file says otherwise
DRUM_CHANNEL = 9         # channel 10: percussion, no pitch


class ScoreError(ValueError):
    pass


# ------------------------------------------------------------------------------------------------------------------ JSON
def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def notes_from_json(items):
    """A list of {"pitch", "velocity", "start", "end"} objects -> [Note]; a missing or ill-typed field is refused by index and name."""
    if not isinstance(items, list):
        raise ScoreError(f"JSON score: a list of note objects is expected (got {type(items).__name__})")
    out = []
    for i, item in enumerate(items):
        if not isinstance(item, dict):
            raise ScoreError(f"JSON score: note {i} is not an object")
        for field, ok, what in (("pitch", _is_int, "an integer MIDI number"), ("velocity", _is_int, "an integer"),
                                ("start", _is_number, "a number of seconds"), ("end", _is_number, "a number of seconds")):
            if field not in item:
                raise ScoreError(f"JSON score: note {i} has no field '{field}'")
            if not ok(item[field]):
                raise ScoreError(f"JSON score: note {i} field '{field}' must be {what} (got {item[field]!r})")
        if not 0 <= item["pitch"] <= 127:
            raise ScoreError(f"JSON score: note {i} field 'pitch' must be 0..127 (got {item['pitch']})")
        if not 1 <= item["velocity"] <= 127:
            raise ScoreError(f"JSON score: note {i} field 'velocity' must be 1..127 (got {item['velocity']})")
        if item["start"] < 0:
            raise ScoreError(f"JSON score: note {i} field 'start' must not be negative (got {item['start']})")
        if not item["start"] < item["end"]:
            raise ScoreError(f"JSON score: note {i} field 'end' must be later than 'start' (got {item['start']} .. {item['end']})")
        out.append(Note(item["pitch"], item["velocity"], float(item["start"]), float(item["end"])))
    order = sorted(range(len(out)), key=lambda i: (out[i].start, i))
    return [out[i] for i in order]


# ------------------------------------------------------------------------------------------------------------------ MIDI
def _vlq(data, pos, end, what):
    """A variable-length quantity at data[pos:end] -> (value, next position)."""
    value = 0
    for _ in range(4):
        if pos >= end:
            raise ScoreError(f"MIDI file: truncated track: {what} runs past the end of its chunk")
        byte = data[pos]
        pos += 1
        value = (value << 7) | (byte & 0x7F)
        if not byte & 0x80:
            return value, pos
    raise ScoreError(f"MIDI file: {what} is longer than four bytes")


def _read_track(data, pos, end, track, counter):
    """One MTrk chunk's events -> ([(pitch, velocity, start tick, end tick, appearance)], [(tick, tempo)])."""
    notes, tempos = [], []
    sounding = {}   # (channel, pitch) -> (start tick, velocity, appearance)
    tick, status = 0, None

    def need(n, what):
        if pos + n > end:
            raise ScoreError(f"MIDI file: truncated track {track}: {what} runs past the end of its chunk")

    def stop(key, at):
        start, velocity, appearance = sounding.pop(key)
        notes.append((key[1], velocity, start, at, appearance))

    while pos < end:
        delta, pos = _vlq(data, pos, end, f"a delta time of track {track}")
        tick += delta
        need(1, "an event")
        if data[pos] & 0x80:
            status = data[pos]
            pos += 1
        elif status is None:
            raise ScoreError(f"MIDI file: track {track} uses running status before any status byte")
        if status == 0xFF:                                   # meta: type, length, payload
            need(1, "a meta event")
            kind = data[pos]
            length, pos = _vlq(data, pos + 1, end, f"a meta event's length in track {track}")
            need(length, "a meta event")
            if kind == 0x51:
                if length != 3:
                    raise ScoreError(f"MIDI file: a tempo event of track {track} has {length} bytes, not 3")
                tempos.append((tick, int.from_bytes(data[pos:pos + 3], "big")))
            pos += length
            status = None                                    # (meta and sysex events cancel running status)
            if kind == 0x2F:
                break
        elif status in (0xF0, 0xF7):                         # sysex: length, payload
            length, pos = _vlq(data, pos, end, f"a sysex event's length in track {track}")
            need(length, "a sysex event")
            pos += length
            status = None
        elif status >= 0xF0:
            raise ScoreError(f"MIDI file: track {track} holds the system message 0x{status:02X}, which a file may not contain")
        else:
            kind, channel = status & 0xF0, status & 0x0F
            size = 1 if kind in (0xC0, 0xD0) else 2
            need(size, "a channel event")
            first, second = data[pos], data[pos + size - 1]
            pos += size
            if kind not in (0x80, 0x90) or channel == DRUM_CHANNEL:
                continue
            key = (channel, first)
            if key in sounding:                              # a note-off, or a re-trigger: the earlier note ends here
                stop(key, tick)
            if kind == 0x90 and second > 0:                  # (note-on with velocity 0 is a note-off)
                sounding[key] = (tick, second, counter[0])
                counter[0] += 1
    for key in sorted(sounding, key=lambda k: sounding[k][2]):   # still sounding: ends at the track's last event
        stop(key, tick)
    return notes, tempos


def notes_from_midi(data):
    """A Standard MIDI File (bytes), format 0 or 1 -> [Note], times in seconds through one tempo map merged over all tracks.  Channel 10
    is skipped; a note-on for a pitch that is sounding on its channel ends the earlier note; a note still sounding at the end of its
    track ends at the track's last event.  (A note that ends at the tick it starts on has no length and is left out.)"""
    data = bytes(data)
    if len(data) < 14 or data[:4] != b"MThd":
        raise ScoreError("MIDI file: truncated or missing MThd header chunk")
    header_len, fmt, ntracks, division = struct.unpack(">IHHH", data[4:14])
    if header_len < 6:
        raise ScoreError(f"MIDI file: MThd chunk of {header_len} bytes (6 expected)")
    if fmt not in (0, 1):
        raise ScoreError(f"MIDI file: format {fmt} is not supported (format 0 or 1 only)")
    if division & 0x8000:
        raise ScoreError("MIDI file: SMPTE division (frames per second) is not supported, only ticks per quarter note")
    if division == 0:
        raise ScoreError("MIDI file: division of 0 ticks per quarter note")
    pos, track, counter = 8 + header_len, 0, [0]
    raw, tempos = [], []
    while track < ntracks:
        if pos + 8 > len(data):
            raise ScoreError(f"MIDI file: truncated: the header announces {ntracks} tracks, the file ends after {track}")
        tag, length = data[pos:pos + 4], int.from_bytes(data[pos + 4:pos + 8], "big")
        pos += 8
        if pos + length > len(data):
            raise ScoreError(f"MIDI file: truncated chunk {tag!r}: {length} bytes announced, {len(data) - pos} present")
        if tag == b"MTrk":
            n, t = _read_track(data, pos, pos + length, track, counter)
            raw += n
            tempos += t
            track += 1
        pos += length                                         # (chunks of another type are skipped by their length)
    # one tempo map: (tick, microseconds per quarter) in tick order; changes at the same tick keep file order, the last one holds
    tempos.sort(key=lambda e: e[0])
    ticks = [0] + [t for t, _ in tempos]
    values = [DEFAULT_TEMPO] + [v for _, v in tempos]
    elapsed = [0]                                             # integer microseconds x division at each change
    for i in range(1, len(ticks)):
        elapsed.append(elapsed[-1] + (ticks[i] - ticks[i - 1]) * values[i - 1])

    def seconds(tick):
        lo, hi = 0, len(ticks)                                # the last change at or before `tick`
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if ticks[mid] <= tick:
                lo = mid
            else:
                hi = mid
        return (elapsed[lo] + (tick - ticks[lo]) * values[lo]) / (division * 1e6)

    out = [(Note(pitch, velocity, seconds(start), seconds(end)), appearance) for pitch, velocity, start, end, appearance in raw if end > start]
    out.sort(key=lambda e: (e[0].start, e[1]))
    return [n for n, _ in out]


def read_notes(path_or_bytes):
    """A score -> [Note] sorted by (start, order of appearance).  `path_or_bytes`: a file name or the file's bytes; a Standard MIDI File is
    recognised by its MThd tag, anything else is read as JSON."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(os.fspath(path_or_bytes), "rb") as f:
            data = f.read()
    if data[:4] == b"MThd":
        return notes_from_midi(data)
    try:
        items = json.loads(data.decode("utf-8"))
    except (UnicodeDecodeError, ValueError) as e:
        raise ScoreError(f"score: neither a Standard MIDI File (no MThd tag) nor JSON ({e})")
    return notes_from_json(items)


# -------------------------------------------------------------------------------------------------------------- schedule
def _round(x):
    return int(math.floor(x + 0.5))


def schedule(notes, pitches, sample_rate, waveform_length, release_seconds):
    """-> (kept notes, table, total samples, dropped).  table[n] = (onset, hold, release, row = n, gain) of kept note n:
        onset = floor(start * sr + 0.5),  hold = clamp(floor((end - start) * sr + 0.5), 1, L),  release = min(R, L - hold),
        gain = velocity / 127,  R = floor(release_seconds * sr + 0.5),  total = max(onset + hold + release).
    Notes whose pitch is not in `pitches` (the label table is sorted(pitches), as dataset.py builds it) are dropped and counted; nothing left
    is a ValueError."""
    sr, length = sample_rate, int(waveform_length)
    if release_seconds < 0:
        raise ValueError(f"schedule: release_seconds must not be negative (got {release_seconds})")
    known = set(pitches)
    full_release = _round(release_seconds * sr)
    kept, table, total = [], [], 0
    for note in sorted(notes, key=lambda n: n.start):   # (stable: equal starts keep their order of appearance)
        if note.pitch not in known:
            continue
        onset = _round(note.start * sr)
        hold = min(max(_round((note.end - note.start) * sr), 1), length)
        release = min(full_release, length - hold)
        table.append((onset, hold, release, len(kept), note.velocity / 127.0))
        kept.append(note)
        total = max(total, onset + hold + release)
    if not kept:
        raise ValueError(f"schedule: none of the {len(notes)} notes has a pitch of the label table "
                         f"({min(known) if known else '-'}..{max(known) if known else '-'})")
    return kept, table, total, len(notes) - len(kept)


def labels_for(kept, pitches):
    """One-hot rows [N, len(pitches)] (fp32, host) of the kept notes in the label table sorted(pitches)."""
    index = {p: i for i, p in enumerate(sorted(pitches))}
    labels = torch.zeros(len(kept), len(index), dtype=torch.float32)
    for n, note in enumerate(kept):
        labels[n, index[note.pitch]] = 1.0
    return labels


def slerp(a, b, t):
    """Spherical interpolation of two vectors in float64: omega = arccos(clip(<a/|a|, b/|b|>, -1, 1)),
    sin((1 - t) omega) / sin(omega) * a + sin(t omega) / sin(omega) * b; plain linear interpolation when sin(omega) < 1e-6."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    omega = np.arccos(np.clip(np.dot(a / np.linalg.norm(a), b / np.linalg.norm(b)), -1.0, 1.0))
    so = np.sin(omega)
    if so < 1e-6:
        return a + t * (b - a)   # (a itself when b == a)
    return np.sin((1.0 - t) * omega) / so * a + np.sin(t * omega) / so * b


def schedule_latents(kept, total, sample_rate, seed, seconds_per_instrument, latent_size=256):
    """[N, latent_size] fp32 (host): K + 1 anchors at times j * seconds_per_instrument, K = floor(total / sr / seconds_per_instrument) + 1,
    drawn from a CPU torch.Generator seeded with `seed`; a note's latent is the slerp of the two anchors around its start."""
    if not seconds_per_instrument > 0:
        raise ValueError(f"schedule_latents: seconds_per_instrument must be positive (got {seconds_per_instrument})")
    k = int(math.floor(total / sample_rate / seconds_per_instrument)) + 1
    generator = torch.Generator(device="cpu").manual_seed(int(seed))
    anchors = torch.randn(k + 1, latent_size, generator=generator, dtype=torch.float32).double().numpy()
    out = np.empty((len(kept), latent_size), dtype=np.float64)
    for n, note in enumerate(kept):
        x = note.start / seconds_per_instrument
        j = min(int(math.floor(x)), k - 1)
        out[n] = slerp(anchors[j], anchors[j + 1], min(x - j, 1.0))
    return torch.from_numpy(out.astype(np.float32))
