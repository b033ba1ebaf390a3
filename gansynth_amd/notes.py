"""Note sequences: the score reader and the schedule of GANSynth.synthesize (host, pure Python; DESIGN.md "Note sequences").

The reference has no renderer: the rules here are this project's own.  A `Note` is (pitch, velocity, start, end) -- a MIDI number, 1..127,
and seconds with 0 <= start < end.  `read_notes` reads a JSON list or a Standard MIDI File (format 0 or 1); `schedule` turns notes into
the sample-exact table that kernels.HipKernels.note_mix mixes; `schedule_latents` gives every note its latent by spherical
interpolation between anchors drawn from a generator of their own (the global RNG, and with it a training run's stream, does not move).

Parts and stereo (DESIGN.md "Parts and stereo"): `read_score` reads the same files into a `Score` -- the same notes, and per note its part
(a MIDI channel under one program, or a JSON "part"), its channel volume and its pan; `schedule_gains` turns them into the two gains of
kernels.HipKernels.note_mix_stereo, `schedule_part_latents` gives every part a latent trajectory of its own.

Controllers (DESIGN.md "Controllers"): `read_performance` reads the same files into a `Performance` -- the Score with the sustain pedal
applied to the note ends, and per part the channel volume, expression and pan events in time order; `schedule_curves` turns those into
one piecewise-linear gain curve per part for kernels.HipKernels.note_mix_curves.

Pitch bend (DESIGN.md "Pitch bend"): `read_bends` reads the same files into per-part (seconds, semitones) events -- the wheel under the
range of RPN 0,0, or JSON "bend" controls; `schedule_bends` turns them into one playback-rate curve per part for
kernels.HipKernels.note_warp, and `bent_notes` names the notes such a curve touches.
"""
import bisect
import collections
import json
import math
import os
import struct

import numpy as np
import torch

Note = collections.namedtuple("Note", ["pitch", "velocity", "start", "end"])
Part = collections.namedtuple("Part", ["channel", "program"])   # (None, None) for the parts of a JSON score
# notes: what read_notes returns; part / volume / pan: one entry per note (pan: a float in [-1, 1], or None where the score sets none)
Score = collections.namedtuple("Score", ["notes", "part", "volume", "pan", "parts"])

DEFAULT_TEMPO = 500000   # microseconds per quarter note until a file says otherwise
DRUM_CHANNEL = 9         # channel 10: percussion, no pitch
DEFAULT_PROGRAM, DEFAULT_VOLUME = 0, 100   # until a program change / a channel volume (CC 7) says otherwise; pan (CC 10) stays unset


class ScoreError(ValueError):
    pass


# ------------------------------------------------------------------------------------------------------------------ JSON
def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def _json_notes(items):
    """The note objects of a JSON score, validated -> [Note] in file order."""
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
    return out


def notes_from_json(items):
    """A list of {"pitch", "velocity", "start", "end"} objects -> [Note]; a missing or ill-typed field is refused by index and name."""
    out = _json_notes(items)
    order = sorted(range(len(out)), key=lambda i: (out[i].start, i))
    return [out[i] for i in order]


def score_from_json(items):
    """notes_from_json's notes with the optional fields "part" (a non-negative integer, default 0), "volume" (0..127, default 100) and
    "pan" (a number in [-1, 1], default unset) -> Score; an ill-typed or out-of-range one is refused by index and name.  The parts are the
    distinct "part" values in ascending order."""
    out = _json_notes(items)
    part, volume, pan = [], [], []
    for i, item in enumerate(items):
        for field, ok, what, default in (("part", lambda v: _is_int(v) and v >= 0, "a non-negative integer", 0),
                                         ("volume", lambda v: _is_int(v) and 0 <= v <= 127, "an integer 0..127", DEFAULT_VOLUME),
                                         ("pan", lambda v: _is_number(v) and -1 <= v <= 1, "a number in [-1, 1]", None)):
            if field in item and not ok(item[field]):
                raise ScoreError(f"JSON score: note {i} field '{field}' must be {what} (got {item[field]!r})")
        part.append(item.get("part", 0))
        volume.append(item.get("volume", DEFAULT_VOLUME))
        pan.append(float(item["pan"]) if "pan" in item else None)
    values = sorted(set(part))
    order = sorted(range(len(out)), key=lambda i: (out[i].start, i))
    return Score([out[i] for i in order], [values.index(part[i]) for i in order], [volume[i] for i in order], [pan[i] for i in order],
                 [Part(None, None) for _ in values])


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


_CONTROLLERS = {7: "volume", 10: "pan", 11: "expression", 64: "pedal"}


_BEND_CONTROLLERS = {101: "rpn_msb", 100: "rpn_lsb", 6: "data_msb", 38: "data_lsb"}   # pitch-bend sensitivity is RPN 0,0 (read_bends)


def _read_track(data, pos, end, track, counter, controls=None, ends=None, bends=None):
    """One MTrk chunk's events -> ([(pitch, velocity, start tick, end tick, appearance, channel)], [(tick, tempo)]).  `controls` (a list)
    also receives, in file order, (tick, channel, what, value) of every program change ("program"), CC 7 ("volume"), CC 10 ("pan"),
    CC 11 ("expression") and CC 64 ("pedal") outside channel 10; `ends` (a list) receives the tick of the track's last event; `bends` (a
    list) receives, in file order, (tick, channel, what, value) of every pitch-bend message ("bend", value = (msb << 7 | lsb) - 8192)
    and of CC 101 / 100 / 6 / 38 ("rpn_msb", "rpn_lsb", "data_msb", "data_lsb") outside channel 10."""
    notes, tempos = [], []
    sounding = {}   # (channel, pitch) -> (start tick, velocity, appearance)
    tick, status = 0, None

    def need(n, what):
        if pos + n > end:
            raise ScoreError(f"MIDI file: truncated track {track}: {what} runs past the end of its chunk")

    def stop(key, at):
        start, velocity, appearance = sounding.pop(key)
        notes.append((key[1], velocity, start, at, appearance, key[0]))

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
                if controls is not None and channel != DRUM_CHANNEL:
                    if kind == 0xC0:
                        controls.append((tick, channel, "program", first & 0x7F))
                    elif kind == 0xB0 and first in _CONTROLLERS:
                        controls.append((tick, channel, _CONTROLLERS[first], second & 0x7F))
                if bends is not None and channel != DRUM_CHANNEL:
                    if kind == 0xE0:
                        bends.append((tick, channel, "bend", ((second & 0x7F) << 7 | (first & 0x7F)) - 8192))
                    elif kind == 0xB0 and first in _BEND_CONTROLLERS:
                        bends.append((tick, channel, _BEND_CONTROLLERS[first], second & 0x7F))
                continue
            key = (channel, first)
            if key in sounding:                              # a note-off, or a re-trigger: the earlier note ends here
                stop(key, tick)
            if kind == 0x90 and second > 0:                  # (note-on with velocity 0 is a note-off)
                sounding[key] = (tick, second, counter[0])
                counter[0] += 1
    for key in sorted(sounding, key=lambda k: sounding[k][2]):   # still sounding: ends at the track's last event
        stop(key, tick)
    if ends is not None:
        ends.append(tick)
    return notes, tempos


def _midi(data, controls=None, pedal=None, bends=None):
    """notes_from_midi's work -> [(Note, appearance, channel, start tick)] sorted by (start, appearance); `controls` as in _read_track, over
    all tracks in (track, file) order.  `pedal` (a dict, read_performance's): the sustain pedal moves the notes' end ticks before they
    become seconds, and the dict receives `extended` (the notes made longer) and `seconds` (the tempo map, tick -> seconds).  `bends` (a
    dict, read_bends'): receives `events` (_read_track's bends over all tracks in (track, file) order) and `seconds`."""
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
    raw, tempos, ends = [], [], []
    bend_events = None if bends is None else []
    while track < ntracks:
        if pos + 8 > len(data):
            raise ScoreError(f"MIDI file: truncated: the header announces {ntracks} tracks, the file ends after {track}")
        tag, length = data[pos:pos + 4], int.from_bytes(data[pos + 4:pos + 8], "big")
        pos += 8
        if pos + length > len(data):
            raise ScoreError(f"MIDI file: truncated chunk {tag!r}: {length} bytes announced, {len(data) - pos} present")
        if tag == b"MTrk":
            n, t = _read_track(data, pos, pos + length, track, counter, controls, ends, bend_events)
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

    raw = [e for e in raw if e[3] > e[2]]
    if bends is not None:
        bends["events"], bends["seconds"] = bend_events, seconds
    if pedal is not None:
        lanes = {}   # channel -> [(tick, down)] in (tick, track, file) order
        for tick, channel, what, value in sorted(controls, key=lambda e: e[0]):
            if what == "pedal":
                lanes.setdefault(channel, []).append((tick, value >= 64))
        new_ends, pedal["extended"] = _apply_pedal([(e[5], e[0], e[2], e[3]) for e in raw], lanes, max(ends, default=0))
        raw = [e[:3] + (end,) + e[4:] for e, end in zip(raw, new_ends)]
        pedal["seconds"] = seconds
    out = [(Note(pitch, velocity, seconds(start), seconds(end)), appearance, channel, start)
           for pitch, velocity, start, end, appearance, channel in raw]
    out.sort(key=lambda e: (e[0].start, e[1]))
    return out


def notes_from_midi(data):
    """A Standard MIDI File (bytes), format 0 or 1 -> [Note], times in seconds through one tempo map merged over all tracks.  Channel 10
    is skipped; a note-on for a pitch that is sounding on its channel ends the earlier note; a note still sounding at the end of its
    track ends at the track's last event.  (A note that ends at the tick it starts on has no length and is left out.)"""
    return [e[0] for e in _midi(data)]


def score_from_midi(data):
    """notes_from_midi's notes with their parts -> Score.  Program changes, channel volume (CC 7) and pan (CC 10) are collected from all
    tracks; for a note, the value in force is that of the last such event on its channel at a tick at or before the note-on's -- a
    controller ON the note's tick applies wherever it stands; among several on one tick (track, file order) decides and the last one
    holds.  Defaults: program 0, volume 100, no pan; pan = clamp((cc10 - 64) / 63, -1, 1).  A note keeps the values it starts with.  A part
    is a distinct (channel, program in force at note-on), numbered in order of first appearance in the notes."""
    return _score_from_midi(data)[0]


def _score_from_midi(data, pedal=None, bends=None):
    """score_from_midi's work -> (Score, every controller event (tick, channel, what, value) in (track, file) order); `pedal` and `bends` as in _midi."""
    controls = []
    rows = _midi(data, controls, pedal, bends)
    lanes = {}   # (channel, what) -> ([tick], [value]) in (tick, track, file) order: the sort is stable and `controls` is in (track, file) order
    for tick, channel, what, value in sorted(controls, key=lambda e: e[0]):
        ticks, values = lanes.setdefault((channel, what), ([], []))
        ticks.append(tick)
        values.append(value)

    def in_force(channel, what, tick, default):
        ticks, values = lanes.get((channel, what), ((), ()))
        i = bisect.bisect_right(ticks, tick)   # the events at or before `tick`
        return values[i - 1] if i else default

    part, volume, pan, parts = [], [], [], []
    for _, _, channel, tick in rows:
        key = Part(channel, in_force(channel, "program", tick, DEFAULT_PROGRAM))
        if key not in parts:
            parts.append(key)
        part.append(parts.index(key))
        volume.append(in_force(channel, "volume", tick, DEFAULT_VOLUME))
        cc10 = in_force(channel, "pan", tick, None)
        pan.append(None if cc10 is None else min(max((cc10 - 64) / 63.0, -1.0), 1.0))
    return Score([e[0] for e in rows], part, volume, pan, parts), controls


def read_notes(path_or_bytes):
    """A score -> [Note] sorted by (start, order of appearance).  `path_or_bytes`: a file name or the file's bytes; a Standard MIDI File is
    recognised by its MThd tag, anything else is read as JSON."""
    return _read(path_or_bytes, notes_from_midi, notes_from_json)


def read_score(path_or_bytes):
    """The same files -> Score: `notes` is exactly read_notes' list, and every note has its part, volume and pan."""
    return _read(path_or_bytes, score_from_midi, score_from_json)


def _read(path_or_bytes, from_midi, from_json):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(os.fspath(path_or_bytes), "rb") as f:
            data = f.read()
    if data[:4] == b"MThd":
        return from_midi(data)
    try:
        items = json.loads(data.decode("utf-8"))
    except (UnicodeDecodeError, ValueError) as e:
        raise ScoreError(f"score: neither a Standard MIDI File (no MThd tag) nor JSON ({e})")
    return from_json(items)


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


# ------------------------------------------------------------------------------------------------------ parts and stereo
def one_part_score(notes):
    """[Note] -> the Score of one part with the default volume and no pan (the notes in the order given)."""
    notes = list(notes)
    return Score(notes, [0] * len(notes), [DEFAULT_VOLUME] * len(notes), [None] * len(notes), [Part(None, None)])


def kept_indices(notes, pitches):
    """The indices into `notes` of the notes `schedule` keeps, in its order (by start, stable)."""
    known = set(pitches)
    return [i for i in sorted(range(len(notes)), key=lambda i: notes[i].start) if notes[i].pitch in known]


def part_positions(score, spread):
    """One position in [-1, 1] per part for the notes WITHOUT a pan: spread * (2 p / (Q - 1) - 1) for the part of rank p among the Q parts
    that have no pan anywhere in the score (0 when Q == 1), and 0 for a part that is panned elsewhere."""
    if isinstance(spread, bool) or not isinstance(spread, (int, float)) or not 0.0 <= spread <= 1.0:   # (NaN fails the comparison)
        raise ValueError(f"schedule_gains: spread must lie in [0, 1] (got {spread!r})")
    panned = {p for p, pan in zip(score.part, score.pan) if pan is not None}
    free = [p for p in range(len(score.parts)) if p not in panned]
    positions = [0.0] * len(score.parts)
    if len(free) > 1:
        for rank, p in enumerate(free):
            positions[p] = float(spread) * (2.0 * rank / (len(free) - 1) - 1.0)
    return positions


def schedule_gains(kept_index, score, spread=0.0):
    """-> [(gain_l, gain_r)] of the notes score.notes[i], i in kept_index: constant-power panning,
        g = (velocity / 127) * (volume / 127),  theta = (pan + 1) * pi / 4,  gain_l = g cos(theta),  gain_r = g sin(theta)
    computed in float64 and rounded once to fp32 (returned as the Python floats of those fp32 values).  A note without a pan sits at
    its part's position (part_positions).  ValueError for a spread outside [0, 1]."""
    positions = part_positions(score, spread)
    out = []
    for i in kept_index:
        g = (score.notes[i].velocity / 127.0) * (score.volume[i] / 127.0)
        pan = score.pan[i] if score.pan[i] is not None else positions[score.part[i]]
        theta = (pan + 1.0) * math.pi / 4.0
        out.append((float(np.float32(g * math.cos(theta))), float(np.float32(g * math.sin(theta)))))
    return out


def schedule_part_latents(kept, part_of_kept, n_parts, total, sample_rate, seed, seconds_per_instrument, latent_size=256):
    """[N, latent_size] fp32 (host): every part its own trajectory.  ONE CPU torch.Generator seeded with `seed` draws [K + 1, latent_size]
    anchors for part 0, then for part 1 and so on (K as in schedule_latents); a note's latent is the slerp of ITS part's two anchors around
    its start, by schedule_latents' rule -- so the rows of part 0 are schedule_latents' rows."""
    if not seconds_per_instrument > 0:
        raise ValueError(f"schedule_part_latents: seconds_per_instrument must be positive (got {seconds_per_instrument})")
    if len(part_of_kept) != len(kept) or any(not 0 <= p < n_parts for p in part_of_kept):
        raise ValueError(f"schedule_part_latents: part_of_kept must name one of the {n_parts} parts for each of the {len(kept)} notes")
    k = int(math.floor(total / sample_rate / seconds_per_instrument)) + 1
    generator = torch.Generator(device="cpu").manual_seed(int(seed))
    anchors = [torch.randn(k + 1, latent_size, generator=generator, dtype=torch.float32).double().numpy() for _ in range(n_parts)]
    out = np.empty((len(kept), latent_size), dtype=np.float64)
    for n, (note, part) in enumerate(zip(kept, part_of_kept)):
        x = note.start / seconds_per_instrument
        j = min(int(math.floor(x)), k - 1)
        out[n] = slerp(anchors[part][j], anchors[part][j + 1], min(x - j, 1.0))
    return torch.from_numpy(out.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ controllers
# DESIGN.md "Controllers": what a score says AFTER a note has started -- channel volume (CC 7), expression (CC 11), pan (CC 10) and the
# sustain pedal (CC 64) -- read into a Performance and turned into one piecewise-linear gain curve per part for
# kernels.HipKernels.note_mix_curves.  Nothing above reads any of it.
# controls: per part the time-ordered (seconds, kind, value), kind "volume" / "expression" (0..127) or "pan" (a float in [-1, 1])
Performance = collections.namedtuple("Performance", ["score", "controls", "pedal_extended"])
MAX_BEND_RANGE, DEFAULT_BEND_RANGE = 24, 2   # semitones: the clamp of a channel's pitch-bend sensitivity, and its value until RPN 0,0 sets one
CONTROL_KINDS = ("volume", "expression", "pan")
DEFAULT_EXPRESSION = 127


def _apply_pedal(notes, lanes, last):
    """The sustain pedal, in whatever unit of time the caller counts (ticks, seconds).  notes: (lane, pitch, start, end) rows;
    lanes: lane -> [(time, down)] in the order that decides (time, then the file's); last: the time of the file's last event.
    The pedal's state at a time is the one after every event of the lane at or before that time.  A note whose end finds its lane's pedal
    down ends at the first pedal-up after that (at the file's last event when none follows), but no later than the next start of a note of
    the same (lane, pitch) after its own start, and no later than `last`.  -> ([end], how many notes became longer)."""
    starts = {}
    for lane, pitch, start, _ in notes:
        starts.setdefault((lane, pitch), []).append(start)
    for key in starts:
        starts[key].sort()
    ends, extended = [], 0
    for lane, pitch, start, end in notes:
        events = lanes.get(lane, [])
        i = bisect.bisect_right([t for t, _ in events], end)   # the events at or before the note's end
        new_end = end
        if i and events[i - 1][1]:
            ups = [t for t, down in events[i:] if not down]
            new_end = ups[0] if ups else last
            own = starts[(lane, pitch)]
            j = bisect.bisect_right(own, start)
            if j < len(own):
                new_end = min(new_end, own[j])
            new_end = max(min(new_end, last), end)
        extended += new_end > end
        ends.append(new_end)
    return ends, extended


def performance_from_midi(data):
    """A Standard MIDI File -> Performance.  CC 7, CC 11, CC 10 and CC 64 are collected from all tracks outside channel 10 and ordered by
    (tick, track, file order) -- score_from_midi's rule.  The pedal is applied in ticks, before the tempo map turns ticks into seconds.
    A part, a (channel, program), receives the events of its channel; pan = clamp((cc10 - 64) / 63, -1, 1) as in score_from_midi."""
    pedal = {}
    score, events = _score_from_midi(data, pedal)
    controls = [[] for _ in score.parts]
    for tick, channel, what, value in sorted(events, key=lambda e: e[0]):   # (stable: (track, file) order inside a tick)
        if what not in CONTROL_KINDS:
            continue
        if what == "pan":
            value = min(max((value - 64) / 63.0, -1.0), 1.0)
        for p, part in enumerate(score.parts):
            if part.channel == channel:
                controls[p].append((pedal["seconds"](tick), what, value))
    return Performance(score, controls, pedal["extended"])


def performance_from_json(obj, bends=None):
    """A JSON list of notes (score_from_json's; no controls), or {"notes": [...], "controls": [{"part", "time", "control", "value"}]}
    -> Performance.  control: "volume" / "expression" (an integer 0..127), "pan" (a number in [-1, 1]) or "pedal" (a bool, or an integer
    0..127 that is down from 64).  "part" names a "part" value of the notes.  With controls a note's own "volume" or "pan" is refused: the
    controls say it.  The pedal is applied in seconds.  ScoreError by index and field name.  A control may also be "bend" (a number of
    semitones in [-24, 24]; DESIGN.md "Pitch bend"): it is checked like the others and does not enter the Performance; `bends` (a list,
    read_bends') receives per part the time-ordered (seconds, semitones)."""
    if isinstance(obj, list):
        score = score_from_json(obj)
        if bends is not None:
            bends[:] = [[] for _ in score.parts]
        return Performance(score, [[] for _ in score.parts], 0)
    if not isinstance(obj, dict):
        raise ScoreError(f"JSON score: a list of note objects or an object with \"notes\" and \"controls\" is expected (got {type(obj).__name__})")
    for key in obj:
        if key not in ("notes", "controls"):
            raise ScoreError(f"JSON score: unknown field '{key}' (an object holds \"notes\" and \"controls\")")
    if "notes" not in obj:
        raise ScoreError("JSON score: the object has no field 'notes'")
    items, entries = obj["notes"], obj.get("controls", [])
    if isinstance(items, list):
        for i, item in enumerate(items):
            for field in ("volume", "pan"):
                if isinstance(item, dict) and field in item:
                    raise ScoreError(f"JSON score: note {i} field '{field}' is not allowed beside \"controls\": a control says it")
    if not isinstance(entries, list):
        raise ScoreError(f"JSON score: field 'controls' must be a list of control objects (got {type(entries).__name__})")
    _json_notes(items)   # (refusals by note index before anything of the controls)
    values = sorted({item.get("part", 0) for item in items if _is_int(item.get("part", 0))})
    score = score_from_json(items)
    checks = {"volume": (lambda v: _is_int(v) and 0 <= v <= 127, "an integer 0..127"),
              "expression": (lambda v: _is_int(v) and 0 <= v <= 127, "an integer 0..127"),
              "pan": (lambda v: _is_number(v) and -1 <= v <= 1, "a number in [-1, 1]"),
              "pedal": (lambda v: isinstance(v, bool) or (_is_int(v) and 0 <= v <= 127), "a bool or an integer 0..127"),
              "bend": (lambda v: _is_number(v) and -MAX_BEND_RANGE <= v <= MAX_BEND_RANGE, "a number of semitones in [-24, 24]")}
    timed = []
    for i, entry in enumerate(entries):
        if not isinstance(entry, dict):
            raise ScoreError(f"JSON score: control {i} is not an object")
        for field in ("part", "time", "control", "value"):
            if field not in entry:
                raise ScoreError(f"JSON score: control {i} has no field '{field}'")
        if not _is_int(entry["part"]) or entry["part"] not in values:
            raise ScoreError(f"JSON score: control {i} field 'part' must name a part of the notes, one of {values} (got {entry['part']!r})")
        if not _is_number(entry["time"]) or entry["time"] < 0:
            raise ScoreError(f"JSON score: control {i} field 'time' must be a non-negative number of seconds (got {entry['time']!r})")
        if not isinstance(entry["control"], str) or entry["control"] not in checks:
            raise ScoreError(f"JSON score: control {i} field 'control' must be one of {sorted(checks)} (got {entry['control']!r})")
        ok, what = checks[entry["control"]]
        if not ok(entry["value"]):
            raise ScoreError(f"JSON score: control {i} field 'value' must be {what} for '{entry['control']}' (got {entry['value']!r})")
        timed.append((float(entry["time"]), values.index(entry["part"]), entry["control"], entry["value"]))
    timed.sort(key=lambda e: e[0])   # (stable: file order inside one time)
    controls, lanes = [[] for _ in score.parts], {}
    if bends is not None:
        bends[:] = [[(time, float(value)) for time, part, kind, value in timed if kind == "bend" and part == p] for p in range(len(score.parts))]
    for time, part, kind, value in timed:
        if kind == "bend":
            continue
        if kind == "pedal":
            lanes.setdefault(part, []).append((time, value is True or (value is not False and value >= 64)))
        else:
            controls[part].append((time, kind, float(value) if kind == "pan" else value))
    last = max([n.end for n in score.notes] + [e[0] for e in timed])
    ends, extended = _apply_pedal([(p, n.pitch, n.start, n.end) for n, p in zip(score.notes, score.part)], lanes, last)
    return Performance(score._replace(notes=[n._replace(end=end) for n, end in zip(score.notes, ends)]), controls, extended)


def read_performance(path_or_bytes):
    """The files of read_score -> Performance(score, controls, pedal_extended): `score` is read_score's, except that the sustain pedal has
    moved note ends (_apply_pedal; `pedal_extended` counts the notes made longer); `controls` holds per part the time-ordered
    (seconds, kind, value) of channel volume, expression and pan.  JSON may also be the object form of performance_from_json."""
    return _read(path_or_bytes, performance_from_midi, performance_from_json)


def plain_performance(score):
    """A Score -> the Performance without a control or a pedal."""
    return Performance(score, [[] for _ in score.parts], 0)


def control_counts(performance):
    """{"volume": n, "expression": n, "pan": n} over all parts."""
    counts = dict.fromkeys(CONTROL_KINDS, 0)
    for events in performance.controls:
        for _, kind, _ in events:
            counts[kind] += 1
    return counts


def schedule_curves(performance, kept_index, sample_rate, ramp_seconds=0.01, stereo=False, spread=0.0):
    """-> (points, first): one piecewise-linear gain curve per part over clip samples at `sample_rate`, for kernels.note_mix_curves.
    points: (pos, v_l, v_r) rows, pos strictly increasing inside a part; part p owns points[first[p]:first[p + 1]] and has at least one.
    Per part the state (volume, expression, pan) starts at (100, 127, part_positions(score, spread)[p]); its target is
        a = (volume / 127) (expression / 127);  stereo: (a cos(theta), a sin(theta)), theta = (pan + 1) pi / 4;  mono: (a, a), pan ignored.
    An event stands at sample floor(seconds * sr + 0.5); the events of one sample collapse to the state after the last.  Events at sample
    0 set the first value without a ramp.  A later sample s starts a linear ramp from the curve's value at s to the new target at s + R,
    R = max(1, floor(ramp_seconds * sr + 0.5)); a ramp still in progress at s is cut there at its interpolated value.  Outside its points
    a curve is constant.  Everything in float64, rounded once to fp32 (returned as the Python floats of those fp32 values).
    `kept_index` (kept_indices'): the notes that sound; it must index the score's notes and does not change the curves, which describe
    the parts.  ValueError for a ramp that is negative or not finite."""
    score = performance.score
    if isinstance(ramp_seconds, bool) or not isinstance(ramp_seconds, (int, float)) or not math.isfinite(ramp_seconds) or ramp_seconds < 0:
        raise ValueError(f"schedule_curves: ramp_seconds must be a finite, non-negative number of seconds (got {ramp_seconds!r})")
    if any(not 0 <= i < len(score.notes) for i in kept_index):
        raise ValueError(f"schedule_curves: kept_index must index the {len(score.notes)} notes of the score")
    positions = part_positions(score, spread)
    ramp = max(1, _round(ramp_seconds * sample_rate))

    def target(state):
        a = (state["volume"] / 127.0) * (state["expression"] / 127.0)
        if not stereo:
            return (a, a)
        theta = (state["pan"] + 1.0) * math.pi / 4.0
        return (a * math.cos(theta), a * math.sin(theta))

    points, first = [], [0]
    for p, events in enumerate(performance.controls):
        state = {"volume": DEFAULT_VOLUME, "expression": DEFAULT_EXPRESSION, "pan": positions[p]}
        groups = []   # [sample, state after its last event] by sample
        for seconds, kind, value in sorted(events, key=lambda e: e[0]):
            if kind == "pan" and not stereo:
                continue
            state = dict(state, **{kind: value})
            s = _round(seconds * sample_rate)
            if groups and groups[-1][0] == s:
                groups[-1][1] = state
            else:
                groups.append([s, state])
        start = {"volume": DEFAULT_VOLUME, "expression": DEFAULT_EXPRESSION, "pan": positions[p]}
        if groups and groups[0][0] == 0:
            start = groups.pop(0)[1]
        curve = [(0,) + target(start)]
        for s, state in groups:
            pos, v = curve[-1][0], curve[-1][1:]
            if s < pos:                                   # a ramp in progress: cut at its interpolated value
                (p0, *v0), (p1, *v1) = curve[-2], curve[-1]
                x = (s - p0) / (p1 - p0)
                v = tuple(a + x * (b - a) for a, b in zip(v0, v1))
                curve.pop()
            if s != curve[-1][0]:
                curve.append((s,) + tuple(v))
            curve.append((s + ramp,) + target(state))
        points += [(pos, float(np.float32(v_l)), float(np.float32(v_r))) for pos, v_l, v_r in curve]
        first.append(len(points))
    return points, first


# ------------------------------------------------------------------------------------------------------------- pitch bend
# DESIGN.md "Pitch bend": the one channel message that changes pitch.  read_bends reads it, schedule_bends turns it into one
# playback-rate curve per part for kernels.HipKernels.note_warp, bent_notes says which notes that curve touches.  Nothing above reads any of it.
BEND_PIECE = 160                       # a ramp is cut into pieces of at most this many samples
BEND_RATIO_MIN, BEND_RATIO_MAX = 0.25, 4.0


def bends_from_midi(data):
    """A Standard MIDI File -> per part (score_from_midi's numbering) the time-ordered (seconds, semitones).  Outside channel 10:
    0xEn lsb msb gives value = (msb << 7 | lsb) - 8192; the channel's range is set through RPN 0,0 -- CC 101 = 0 and CC 100 = 0 select it
    (127, 127 or anything else deselects), CC 6 then sets its semitones and CC 38 its cents -- starts at 2 semitones and is clamped to
    [0, 24]; semitones = value / 8192 * range, from the value and the range in force, and a bend as well as a change of the range sets a
    new target.  Events are ordered by (tick, track, file order); a part, a (channel, program), receives the events of its channel."""
    found = {}
    score, _ = _score_from_midi(data, None, found)
    state = {}   # channel -> [rpn msb, rpn lsb, range semitones, range cents, value]
    out = [[] for _ in score.parts]
    for tick, channel, what, value in sorted(found["events"], key=lambda e: e[0]):   # (stable: (track, file) order inside a tick)
        st = state.setdefault(channel, [127, 127, DEFAULT_BEND_RANGE, 0, 0])
        if what == "rpn_msb":
            st[0] = value
            continue
        if what == "rpn_lsb":
            st[1] = value
            continue
        if what == "bend":
            st[4] = value
        elif (st[0], st[1]) != (0, 0):
            continue                                     # data entry for another parameter
        elif what == "data_msb":
            st[2] = value
        else:
            st[3] = value
        span = min(max(st[2] + st[3] / 100.0, 0.0), float(MAX_BEND_RANGE))
        for p, part in enumerate(score.parts):
            if part.channel == channel:
                out[p].append((found["seconds"](tick), st[4] / 8192.0 * span))
    return out


def bends_from_json(obj):
    """performance_from_json's files -> per part the time-ordered (seconds, semitones) of their "bend" controls (a list of notes has none)."""
    out = []
    performance_from_json(obj, out)
    return out


def read_bends(path_or_bytes):
    """The files of read_score -> per part, in read_score's numbering, the time-ordered [(seconds, semitones)] of its pitch bend."""
    return _read(path_or_bytes, bends_from_midi, bends_from_json)


def schedule_bends(bends, sample_rate, ramp_seconds=0.01):
    """-> (points, first), all float64: one playback-rate curve per part over clip samples at `sample_rate`, for kernels.note_warp.
    points: (pos, ratio, cum) rows, pos strictly increasing inside a part; part p owns points[first[p]:first[p + 1]], and a part without
    a bend event owns none.  schedule_curves' conventions, in semitones: an event stands at floor(seconds * sr + 0.5), the events of one
    sample collapse to the last, events at sample 0 set the value (0 otherwise) without a ramp, a later one starts a linear ramp of
    R = max(1, floor(ramp_seconds * sr + 0.5)) samples from the curve's value there, and a ramp in progress is cut at its interpolated
    value.  A ramp longer than 160 samples is cut into pieces of at most 160.  ratio = clamp(2 ** (semitones / 12), 0.25, 4); between
    points the RATIO is linear in clip samples, outside them constant; cum = Phi(pos), Phi(t) the integral of the ratio from 0 to t, by
        Phi(t) = cum_i + ratio_i * d + (ratio_{i+1} - ratio_i) * d * d / (2 * (pos_{i+1} - pos_i)),   d = t - pos_i
    in float64 in this order.  ValueError for a ramp that is negative or not finite, and for an event that is not (seconds >= 0, finite
    semitones)."""
    if isinstance(ramp_seconds, bool) or not isinstance(ramp_seconds, (int, float)) or not math.isfinite(ramp_seconds) or ramp_seconds < 0:
        raise ValueError(f"schedule_bends: ramp_seconds must be a finite, non-negative number of seconds (got {ramp_seconds!r})")
    ramp = max(1, _round(ramp_seconds * sample_rate))
    points, first = [], [0]
    for p, events in enumerate(bends):
        groups = []   # [sample, semitones after its last event] by sample
        for e in events:
            if len(e) != 2 or not all(_is_number(v) for v in e) or e[0] < 0:
                raise ValueError(f"schedule_bends: part {p} holds {e!r}, not (seconds >= 0, semitones)")
        for seconds, semitones in sorted(events, key=lambda e: e[0]):
            s = _round(seconds * sample_rate)
            if groups and groups[-1][0] == s:
                groups[-1][1] = float(semitones)
            else:
                groups.append([s, float(semitones)])
        if not groups:
            first.append(len(points))
            continue
        start = groups.pop(0)[1] if groups[0][0] == 0 else 0.0
        curve = [(0, start)]
        for s, target in groups:
            v = curve[-1][1]
            if s < curve[-1][0]:                          # a ramp in progress: cut at its interpolated value
                (p0, v0), (p1, v1) = curve[-2], curve[-1]
                v = v0 + (s - p0) / (p1 - p0) * (v1 - v0)
                curve.pop()
            if s != curve[-1][0]:
                curve.append((s, v))
            curve.append((s + ramp, target))
        fine = [curve[0]]
        for (p0, v0), (p1, v1) in zip(curve, curve[1:]):
            if v0 != v1:
                fine += [(pos, v0 + (pos - p0) / (p1 - p0) * (v1 - v0)) for pos in range(p0 + BEND_PIECE, p1, BEND_PIECE)]
            fine.append((p1, v1))
        cum = 0.0
        for i, (pos, semitones) in enumerate(fine):
            ratio = min(max(2.0 ** (semitones / 12.0), BEND_RATIO_MIN), BEND_RATIO_MAX)
            if i:
                p0, r0, _ = points[-1]
                d = float(pos) - p0
                cum = cum + r0 * d + (ratio - r0) * d * d / (2.0 * d)
            points.append((float(pos), ratio, cum))
        first.append(len(points))
    return points, first


def bent_notes(table, part_of_note, points, first):
    """The indices of the notes of `table` (schedule's rows; part_of_note: their parts) whose part's ratio differs from 1 anywhere in
    [onset, onset + hold + release): the ratio is piecewise linear, so it does where it differs at an end of the span or at a point
    inside it."""
    out, curves = [], {}   # part -> (its points, their positions)
    for n, (row, p) in enumerate(zip(table, part_of_note)):
        if p not in curves:
            pts = points[first[p]:first[p + 1]]
            curves[p] = (pts, [q[0] for q in pts])
        pts, pos = curves[p]
        if not pts:
            continue
        lo, hi = row[0], row[0] + row[1] + row[2] - 1

        def ratio(t):
            k = bisect.bisect_right(pos, t)
            if k == 0 or k == len(pts):
                return pts[max(k - 1, 0)][1]
            (p0, r0, _), (p1, r1, _) = pts[k - 1], pts[k]
            return r0 + (r1 - r0) * (t - p0) / (p1 - p0)

        i0, i1 = bisect.bisect_left(pos, lo), bisect.bisect_right(pos, hi)
        if ratio(lo) != 1.0 or ratio(hi) != 1.0 or any(pts[i][1] != 1.0 for i in range(i0, i1)):
            out.append(n)
    return out


# ---------------------------------------------------------------------------------------------------------------- sustain
# DESIGN.md "Sustain": notes the score holds longer than the generated waveform.  sustain_plan says where a note's loop is searched,
# pick_loop picks its length from the scores of kernels.HipKernels.loop_search, schedule_sustain cuts a held note into pieces the mix
# accepts, each a row that kernels.HipKernels.note_sustain writes.  Nothing above reads any of it.
def sustain_plan(waveform_length):
    """-> (a, m_min, m_max, W, X) for notes of L = waveform_length samples: the loop starts at a = 3 L // 8, its length lies in
    [L // 8, L // 4], a lag is scored over a window of W = max(16, L // 32) samples and a wrap is crossfaded over X = max(1, L // 64).
    a + m_max + max(W, X) <= L for every L >= 64; a smaller L is a ValueError."""
    length = int(waveform_length)
    if length < 64:
        raise ValueError(f"sustain_plan: the waveform must have at least 64 samples (got {waveform_length})")
    return 3 * length // 8, length // 8, length // 4, max(16, length // 32), max(1, length // 64)


def pick_loop(scores, m_min, tie=1e-3):
    """The loop length from the scores of the lags m_min, m_min + 1, ...: the LARGEST lag whose score is at least max - tie (every
    multiple of the period scores near 1 and a longer loop repeats less audibly, so the margin, not rounding, decides between them).
    Non-finite scores count as -inf; where every score is -inf or 0 the note is silent and the largest lag is taken."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    if s.size == 0:
        raise ValueError("pick_loop: no scores")
    s = np.where(np.isfinite(s), s, -np.inf)
    if np.all((s == 0.0) | np.isneginf(s)):
        return int(m_min) + s.size - 1
    return int(m_min) + int(np.nonzero(s >= s.max() - tie)[0][-1])


def sustain_pieces(hold, full_release, waveform_length):
    """A hold of `hold` samples followed by the full release R (hold + R > L, R <= L - 1) -> [(offset, hold_s, release_s)], pieces that
    tile [0, hold) and that the mix accepts (hold_s >= 1, hold_s + release_s <= L), only the last with a release: pieces of L while more
    than L remains; a remainder r <= L - R is the last piece, a longer one is split into r - (L - R) and L - R."""
    length, out, offset = int(waveform_length), [], 0
    while hold - offset > length:
        out.append((offset, length, 0))
        offset += length
    r = hold - offset
    if r > length - full_release:
        out.append((offset, r - (length - full_release), 0))
        offset, r = offset + r - (length - full_release), length - full_release
    out.append((offset, r, full_release))
    return out


def schedule_sustain(notes, pitches, sample_rate, waveform_length, release_seconds, cut=()):
    """`schedule` for notes that may be held past the waveform -> (kept notes, table, total samples, dropped, owner, offset).
    hold = max(1, floor((end - start) * sr + 0.5)), unclamped; a note is HELD iff hold + R > L.  Every other note -- and every kept
    note whose index is in `cut` -- gets exactly schedule's row.  A held note keeps its full release R and becomes one table entry per
    piece of sustain_pieces: (onset + offset_s, hold_s, release_s, a row of its own, the note's gain); the rows of the pieces count on
    from N = len(kept) in table order, and under the mix's envelope -- 1 over a hold -- the pieces butt together sample-exactly.
    owner[e] is the kept note of table entry e; offset[e] is the piece's offset into the held note, None for an ordinary row.
    R <= L - 1 is required (ValueError): a piece with a release needs a hold of at least one sample."""
    sr, length = sample_rate, int(waveform_length)
    kept, table, total, dropped = schedule(notes, pitches, sr, length, release_seconds)
    full_release = _round(release_seconds * sr)
    if full_release > length - 1:
        raise ValueError(f"schedule_sustain: the release of {full_release} samples must be at most {length - 1}, the waveform's "
                         f"length less one (release_seconds {release_seconds})")
    cut = set(cut)
    out, owner, offset, next_row = [], [], [], len(kept)
    for n, (note, row) in enumerate(zip(kept, table)):
        hold = max(_round((note.end - note.start) * sr), 1)
        if hold + full_release <= length or n in cut:
            out.append(row)
            owner.append(n)
            offset.append(None)
            continue
        for piece_offset, piece_hold, piece_release in sustain_pieces(hold, full_release, length):
            out.append((row[0] + piece_offset, piece_hold, piece_release, next_row, row[4]))
            owner.append(n)
            offset.append(piece_offset)
            total = max(total, row[0] + piece_offset + piece_hold + piece_release)
            next_row += 1
    return kept, out, total, dropped, owner, offset
