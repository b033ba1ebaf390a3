"""CPU: the host layers of parts and stereo (DESIGN.md "Parts and stereo") -- read_score on MIDI bytes assembled here and on JSON, the
gains and the per-part latents against tests/stereo_ref.py, the refusals of gs_note_mix_stereo and gs_stereo_finish (no launch), the
table validation of kernels.note_mix_stereo, the driver's flags and the signature of GANSynth.synthesize."""
import ctypes
import inspect
import json
import math

import numpy as np
import pytest
import torch

from tests import stereo_ref as STR
from tests import synth_ref as SRF
from tests.test_notes_cpu import END, format0_file, header, tempo, track


# ---------------------------------------------------------------------------------------------------------- the reader
def quartet_file():
    """Format 1, 480 ticks per quarter at the default tempo (960 ticks a second): a conductor track, channel 1 with a program change in
    mid-file, channel 2 with pans, and a track that holds channel 3, channel 10 and a controller of channel 1."""
    conductor = track([(0, tempo(500000)), (0, [0xFF, 0x58, 0x04, 4, 2, 24, 8]), (0, END)])
    one = track([
        (0, [0xC0, 40]),                # tick 0     program 40
        (0, [0xB0, 7, 90]),             #            volume 90
        (0, [10, 0]),                   #            running status: CC 10 = 0, pan clamps to -1
        (0, [0x90, 60, 100]),           #            A on: program 40, volume 90, pan -1
        (240, [0x80, 60, 0]),           # tick 240   A off
        (240, [0x90, 62, 80]),          # tick 480   B on ...
        (0, [0xB0, 7, 50]),             #            ... and a volume on the same tick, after the note in the file: it applies
        (0, [7, 60]),                   #            running status, the same tick again: the later one holds (in this track)
        (120, [0xB0, 7, 20]),           # tick 600   after B's tick: B keeps what it started with
        (120, [0x80, 62, 0]),           # tick 720   B off
        (0, [0xC0, 41]),                #            a program change in mid-file: a new part
        (0, [0x90, 64, 70]),            #            C on: program 41, volume 20, pan -1
        (240, [0x80, 64, 0]),           # tick 960
        (0, END)])
    two = track([
        (0, [0x91, 48, 64]),            # tick 0     D on: no program, no volume, no pan yet
        (100, [0xB1, 10, 127]),         # tick 100   pan +1
        (380, [0x91, 50, 64]),          # tick 480   E on ...
        (0, [0xB1, 10, 64]),            #            ... and the pan of the same tick: centre
        (200, [0x81, 48, 0]),           # tick 680   D off
        (0, [50, 0]),                   #            E off by running status
        (0, END)])
    three = track([
        (0, [0xB9, 7, 1]),              # channel 10: volume, pan by running status, program -- all ignored
        (0, [10, 127]),
        (0, [0xC9, 5]),
        (0, [0x99, 36, 100]),           # a drum note: skipped
        (0, [0x92, 72, 127]),           # tick 0     F on, channel 3
        (480, [0xB0, 7, 70]),           # tick 480   a volume for CHANNEL 1 from a later track: the last of that tick, so B has it
        (0, [0x82, 72, 0]),             #            F off
        (0, [0x89, 36, 0]),
        (0, END)])
    return header(1, 4, 480) + conductor + one + two + three


def test_midi_score():
    from gansynth_amd import notes as N
    data = quartet_file()
    score = N.read_score(data)
    assert isinstance(score, N.Score) and score.notes == N.read_notes(data)
    assert [(n.pitch, n.velocity) for n in score.notes] == [(60, 100), (48, 64), (72, 127), (62, 80), (50, 64), (64, 70)]   # A D F B E C
    assert [n.start for n in score.notes] == [0.0, 0.0, 0.0, 0.5, 0.5, 0.75]
    assert score.parts == [N.Part(0, 40), N.Part(1, 0), N.Part(2, 0), N.Part(0, 41)] and all(isinstance(p, N.Part) for p in score.parts)
    assert score.part == [0, 1, 2, 0, 1, 3]
    assert score.volume == [90, 100, 100, 70, 100, 20]
    assert score.pan == [-1.0, None, None, -1.0, 0.0, -1.0]
    # a pan between the ends: (cc10 - 64) / 63
    one = header(0, 1, 96) + track([(0, [0xB3, 10, 96]), (0, [0x93, 60, 1]), (96, [0x83, 60, 0]), (0, [0xB3, 10, 127]), (0, END)])
    score = N.read_score(one)
    assert score.pan == [32 / 63] and score.parts == [N.Part(3, 0)] and score.volume == [100] and score.notes == N.read_notes(one)


def test_score_notes_are_read_notes(tmp_path):
    from gansynth_amd import notes as N
    two_tracks = header(1, 2, 96) + track([(0, tempo(1000000)), (96, tempo(500000)), (0, END)]) + \
        track([(0, [0x91, 48, 64]), (48, [0x90, 55, 1]), (144, [0x81, 48, 0]), (96, [0x80, 55, 0]), (0, END)])
    items = [dict(pitch=60, velocity=100, start=0.5, end=1.0), dict(pitch=62, velocity=5, start=0.0, end=2.0),
             dict(pitch=64, velocity=127, start=0.5, end=0.75, part=2, pan=-0.5)]
    path = tmp_path / "score.json"
    path.write_text(json.dumps(items))
    for source in (format0_file(), two_tracks, quartet_file(), json.dumps(items).encode(), path):
        score = N.read_score(source)
        assert score.notes == N.read_notes(source)
        assert len(score.part) == len(score.volume) == len(score.pan) == len(score.notes) and max(score.part) == len(score.parts) - 1
    score = N.read_score(format0_file())        # one channel, no controller: one part with the defaults
    assert score.parts == [N.Part(0, 0)] and set(score.part) == {0} and set(score.volume) == {100} and set(score.pan) == {None}
    assert N.read_score(two_tracks).parts == [N.Part(1, 0), N.Part(0, 0)]
    with pytest.raises(ValueError, match="SMPTE"):
        N.read_score(header(0, 1, 0xE728) + track([(0, END)]))


def test_json_score():
    from gansynth_amd import notes as N
    items = [dict(pitch=60, velocity=100, start=0.5, end=1.0, part=7, volume=64),
             dict(pitch=62, velocity=5, start=0.0, end=2.0, pan=0.25),
             dict(pitch=64, velocity=127, start=0.5, end=0.75, part=3, pan=-1, volume=0),
             dict(pitch=65, velocity=1, start=0.25, end=0.75, part=7)]
    score = N.read_score(json.dumps(items).encode())
    assert score.notes == [N.Note(62, 5, 0.0, 2.0), N.Note(65, 1, 0.25, 0.75), N.Note(60, 100, 0.5, 1.0), N.Note(64, 127, 0.5, 0.75)]
    assert score.parts == [N.Part(None, None)] * 3           # the distinct values 0, 3, 7 in ascending order
    assert score.part == [0, 2, 2, 1] and score.volume == [100, 100, 64, 0] and score.pan == [0.25, None, None, -1.0]
    plain = N.read_score(json.dumps([{k: v for k, v in item.items() if k in ("pitch", "velocity", "start", "end")} for item in items]).encode())
    assert plain.notes == score.notes and plain.parts == [N.Part(None, None)] and set(plain.part) == {0} and set(plain.pan) == {None}
    for field, value in (("part", -1), ("part", 1.5), ("part", "violin"), ("part", True), ("volume", 128), ("volume", -1), ("volume", 64.0),
                         ("volume", None), ("pan", 1.01), ("pan", -2), ("pan", "left"), ("pan", None), ("pan", float("nan"))):
        bad = [dict(items[0]), dict(items[1]), dict(items[3], **{field: value})]
        with pytest.raises(ValueError, match=rf"note 2 .*'{field}'"):
            N.read_score(json.dumps(bad).encode())
        assert len(N.read_notes(json.dumps(bad).encode())) == 3        # read_notes does not look at them, as before
    with pytest.raises(ValueError, match=r"note 1 .*'velocity'"):        # the required fields, refused as read_notes refuses them
        N.read_score(json.dumps([dict(items[0]), dict(pitch=60, start=0.0, end=1.0)]).encode())


# ---------------------------------------------------------------------------------------------------------- the gains
def _score(N, rows, n_parts):
    """rows: (velocity, volume, pan, part)."""
    notes = [N.Note(60, v, 0.1 * i, 0.1 * i + 0.5) for i, (v, _, _, _) in enumerate(rows)]
    return N.Score(notes, [r[3] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [N.Part(None, None)] * n_parts)


def test_schedule_gains():
    from gansynth_amd import notes as N
    rows = [(127, 127, 0.0, 0), (100, 90, -1.0, 0), (64, 100, 1.0, 1), (1, 0, 0.3, 1), (90, 127, None, 2), (77, 50, None, 3), (127, 1, None, 4)]
    score = _score(N, rows, 5)
    for spread in (0.0, 0.5, 1.0):
        got = N.schedule_gains(range(7), score, spread)
        want = STR.gains(*zip(*rows), 5, spread)
        assert len(got) == 7 and all(isinstance(g, float) for pair in got for g in pair)
        assert [(np.float32(l), np.float32(r)) for l, r in got] == want and [(float(l), float(r)) for l, r in want] == got
    # the ends and the centre, by the rule itself
    got = N.schedule_gains(range(7), score, 1.0)
    assert got[0] == (float(np.float32(math.cos(math.pi / 4))), float(np.float32(math.sin(math.pi / 4))))
    assert got[1][0] == float(np.float32(100 / 127 * (90 / 127))) and got[1][1] == 0.0          # hard left
    assert abs(got[2][0]) < 1e-16 and got[2][1] == float(np.float32(64 / 127 * (100 / 127)))    # hard right (cos(pi / 2) in float64)
    assert got[3] == (0.0, 0.0)                                                              # volume 0
    # parts 2, 3, 4 have no pan anywhere: at spread 1 they sit at -1, 0, +1; parts 0 and 1 are where their pans put them
    assert got[4][1] == 0.0 and got[5][0] == got[5][1] and abs(got[6][0]) < 1e-16
    assert N.part_positions(score, 0.5) == [0.0, 0.0, -0.5, 0.0, 0.5]
    for (vel, vol, _, _), (l, r) in zip(rows, got):                                          # constant power
        assert abs(math.hypot(l, r) - vel / 127 * vol / 127) <= 2.0 ** -23
    # a subset and another order: the gains follow kept_index
    assert N.schedule_gains([5, 0], score, 0.5) == [N.schedule_gains(range(7), score, 0.5)[i] for i in (5, 0)]
    # no part is panned: all Q = 3 fan out; one part: the centre whatever the spread
    free = _score(N, [(127, 127, None, 0), (127, 127, None, 1), (127, 127, None, 2), (127, 127, None, 1)], 3)
    assert N.part_positions(free, 0.8) == [-0.8, 0.0, 0.8]
    assert [(np.float32(l), np.float32(r)) for l, r in N.schedule_gains(range(4), free, 0.8)] == STR.gains([127] * 4, [127] * 4, [None] * 4, [0, 1, 2, 1], 3, 0.8)
    solo = _score(N, [(127, 127, None, 0), (90, 100, None, 0)], 1)
    assert N.schedule_gains(range(2), solo, 1.0) == N.schedule_gains(range(2), solo, 0.0) and N.part_positions(solo, 1.0) == [0.0]
    # a note without a pan in a part that is panned elsewhere: the centre, and the part does not count among the Q
    mixed = _score(N, [(127, 127, None, 0), (127, 127, 0.5, 0), (127, 127, None, 1), (127, 127, None, 2)], 3)
    assert N.part_positions(mixed, 1.0) == [0.0, -1.0, 1.0]
    assert [(np.float32(l), np.float32(r)) for l, r in N.schedule_gains(range(4), mixed, 1.0)] == \
        STR.gains([127] * 4, [127] * 4, [None, 0.5, None, None], [0, 0, 1, 2], 3, 1.0)
    for spread in (-0.01, 1.01, float("nan"), float("inf"), None, "wide"):
        with pytest.raises(ValueError, match="spread"):
            N.schedule_gains(range(7), score, spread)
    # the one-part score of a plain list, and the indices schedule keeps
    notes = [N.Note(60, 100, 0.5, 1.0), N.Note(20, 100, 0.0, 1.0), N.Note(62, 50, 0.25, 0.5), N.Note(64, 127, 0.5, 0.6)]
    one = N.one_part_score(notes)
    assert one.notes == notes and one.parts == [N.Part(None, None)] and one.volume == [100] * 4 and one.pan == [None] * 4
    index = N.kept_indices(notes, range(24, 85))
    kept, _, _, dropped = N.schedule(notes, range(24, 85), 16000, 1024, 0.01)
    assert index == [2, 0, 3] and [notes[i] for i in index] == kept and dropped == 1


# --------------------------------------------------------------------------------------------------------- the latents
def test_part_latents():
    from gansynth_amd import notes as N
    kept = [N.Note(60, 100, s, s + 0.5) for s in (0.0, 2.5, 6.0, 6.0, 11.9, 13.0)]
    parts = [0, 1, 0, 1, 2, 0]
    total = int(13.5 * 16000)
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    lat = N.schedule_part_latents(kept, parts, 3, total, 16000, 5, 6.0)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert lat.shape == (6, 256) and lat.dtype == torch.float32
    mono = N.schedule_latents(kept, total, 16000, 5, 6.0)
    assert torch.equal(lat[[0, 2, 5]], mono[[0, 2, 5]])                      # part 0 is schedule_latents' trajectory
    assert torch.equal(N.schedule_part_latents(kept, [0] * 6, 1, total, 16000, 5, 6.0), mono)
    assert not torch.equal(lat[2], lat[3]) and not torch.equal(lat[1], mono[1]) and not torch.equal(lat[4], mono[4])   # the same start, two parts
    assert torch.equal(N.schedule_part_latents(kept, parts, 3, total, 16000, 5, 6.0), lat)
    # one generator, the parts' anchors drawn one after the other
    k = int(13.5 // 6.0) + 1
    g = torch.Generator().manual_seed(5)
    anchors = [torch.randn(k + 1, 256, generator=g).double().numpy() for _ in range(3)]
    for n, (note, p) in enumerate(zip(kept, parts)):
        want = SRF.note_latents(anchors[p], [note.start], 6.0)[0]
        assert np.abs(lat[n].numpy() - want).max() <= 1e-6, n
    assert torch.equal(lat[3], torch.from_numpy(anchors[1][1].astype(np.float32)))    # a note on an anchor is that anchor
    with pytest.raises(ValueError):
        N.schedule_part_latents(kept, parts, 2, total, 16000, 5, 6.0)                  # part 2 of 2
    with pytest.raises(ValueError):
        N.schedule_part_latents(kept, parts, 3, total, 16000, 5, 0.0)


# ---------------------------------------------------------------------------------------------------- ABI without a GPU
def test_stereo_note_mirror():
    from gansynth_amd import _lib
    assert ctypes.sizeof(_lib.GsMixNoteStereo) == 32
    assert [(n, getattr(_lib.GsMixNoteStereo, n).offset) for n, _ in _lib.GsMixNoteStereo._fields_] == \
        [("onset", 0), ("hold", 8), ("release", 12), ("row", 16), ("gain_l", 20), ("gain_r", 24), ("reserved", 28)]


def test_note_mix_stereo_refusals_without_gpu():
    from gansynth_amd import _lib
    lib = _lib.load()
    P = 0x10000   # (never dereferenced: the argument checks come first and nothing is launched)
    good = dict(waves=P, rows=4, length=1024, row_stride=1024, notes=P, n_notes=3, total=5000, normalize=1, out=P, out_stride=5000, pcm=None,
                peak=None, ws=P, ws_bytes=1 << 20, stream=None)
    order = list(good)
    bad = [("n_notes", 0, b"n_notes"), ("n_notes", -2, b"n_notes"), ("total", 0, b"total"), ("total", -1, b"total"), ("rows", 0, b"rows"),
           ("length", 0, b"length"), ("row_stride", 1023, b"row_stride"), ("out_stride", 4999, b"out_stride"), ("waves", None, b"null"),
           ("notes", None, b"null"), ("out", None, b"null"), ("notes", P + 4, b"notes must be 8-byte"), ("pcm", P + 1, b"pcm must be 2-byte"),
           ("out", P + 2, b"4-byte"), ("ws_bytes", 4, b"workspace"), ("ws", None, b"workspace")]
    for field, value, message in bad:
        args = dict(good, **{field: value})
        assert lib.gs_note_mix_stereo(*[args[k] for k in order]) == -1, (field, value)       # GS_ERR_ARG
        assert message in lib.gs_last_error() and b"note_mix_stereo" in lib.gs_last_error(), (field, value, lib.gs_last_error())
    for nbytes in (lib.gs_note_mix_stereo_workspace_bytes, lib.gs_stereo_finish_workspace_bytes):      # one |max| per tile of both rows
        assert nbytes(0) == 0 and nbytes(-5) == 0
        assert nbytes(1) == 4 and nbytes(_lib.MIX_TILE) == 4 and nbytes(_lib.MIX_TILE + 1) == 8 and nbytes(960000) == 4 * -(-960000 // _lib.MIX_TILE)
        assert nbytes(1 << 33) > nbytes(1 << 32)


def test_stereo_finish_refusals_without_gpu():
    from gansynth_amd import _lib
    lib = _lib.load()
    P = 0x10000
    good = dict(x=P, n=5000, row_stride=5000, normalize=1, pcm=None, peak=None, ws=P, ws_bytes=1 << 20, stream=None)
    order = list(good)
    bad = [("n", 0, b"n must be positive"), ("n", -3, b"n must be positive"), ("row_stride", 4999, b"row_stride"), ("x", None, b"null"),
           ("x", P + 2, b"4-byte"), ("pcm", P + 1, b"pcm must be 2-byte"), ("ws_bytes", 4, b"workspace"), ("ws", None, b"workspace")]
    for field, value, message in bad:
        args = dict(good, **{field: value})
        assert lib.gs_stereo_finish(*[args[k] for k in order]) == -1, (field, value)
        assert message in lib.gs_last_error() and b"stereo_finish" in lib.gs_last_error(), (field, value, lib.gs_last_error())
    assert lib.gs_stereo_finish(*[dict(good, normalize=0)[k] for k in order]) == 0           # nothing is asked for: nothing is launched


def test_note_mix_stereo_table_validation():
    from gansynth_amd import kernels
    good = [(100, 50, 10, 1, 0.5, 0.25), (0, 64, 0, 0, 1.0, 0.0), (100, 1, 63, 2, 0.25, 0.75)]
    arr = kernels.note_mix_stereo_table(good, rows=3, length=64, total=200)
    assert [(n.onset, n.hold, n.release, n.row, n.gain_l, n.gain_r, n.reserved) for n in arr] == \
        [(0, 64, 0, 0, 1.0, 0.0, 0), (100, 50, 10, 1, 0.5, 0.25, 0), (100, 1, 63, 2, 0.25, 0.75, 0)]
    for field, value in (("onset", -1), ("onset", 200), ("hold", 0), ("hold", 65), ("release", -1), ("release", 15), ("row", 3), ("row", -1),
                         ("gain_l", float("nan")), ("gain_r", float("inf")), ("gain_r", None), ("gain_l", True), ("hold", 2.5)):
        entry = dict(zip(("onset", "hold", "release", "row", "gain_l", "gain_r"), good[0]))
        entry[field] = value
        with pytest.raises(ValueError, match=rf"note_mix_stereo: note 1 field '{field}'"):
            kernels.note_mix_stereo_table([good[1], tuple(entry.values()), good[2]], rows=3, length=64, total=200)
    with pytest.raises(ValueError, match="empty"):
        kernels.note_mix_stereo_table([], rows=3, length=64, total=200)
    with pytest.raises(ValueError, match="note 0 has 5 fields"):                 # a mono row
        kernels.note_mix_stereo_table([(0, 64, 0, 0, 1.0)], rows=3, length=64, total=200)


def test_note_mix_stereo_validates_before_the_library_call(monkeypatch):
    """kernels.note_mix_stereo refuses a bad table on the host: the library is not reached (its call is patched to say so)."""
    from gansynth_amd import kernels

    class Lib:
        def __getattr__(self, name):
            raise AssertionError(f"{name} reached")

    K = kernels.HipKernels.__new__(kernels.HipKernels)
    K.lib = Lib()
    waves = torch.zeros(3, 64)
    with pytest.raises(ValueError, match=r"note 1 field 'gain_r'"):
        K.note_mix_stereo(waves, [(0, 64, 0, 0, 1.0, 0.0), (5, 10, 0, 1, 0.5, float("nan"))], 200)
    with pytest.raises(ValueError, match=r"note 0 field 'row'"):
        K.note_mix_stereo(waves, [(0, 64, 0, 3, 1.0, 0.0)], 200)
    with pytest.raises(ValueError, match="waves must be"):
        K.note_mix_stereo(waves.double(), [(0, 64, 0, 0, 1.0, 0.0)], 200)
    with pytest.raises(ValueError, match="stereo_finish: x must be"):
        K.stereo_finish(torch.zeros(2, 8))                                        # not on the device
    with pytest.raises(AssertionError, match="gs_note_mix_stereo_workspace_bytes reached"):   # a good table goes on to the library
        K.note_mix_stereo(waves, [(0, 64, 0, 0, 1.0, 0.0)], 200)


# -------------------------------------------------------------------------------------- the bound, on the GPU test's tables
@pytest.mark.parametrize("lean", [0.2, 0.8])
def test_fp32_evaluation_sits_inside_the_bound(lean):
    """The tables of tests/test_ensemble_gpu.py: an fp32 evaluation in the stated order stays inside (M + 6) 2^-24 A on both channels, and
    the draw has what it is meant to have -- three tiles, the last one partial, a dozen notes on one sample, both peaks above 1 and the
    louder side where `lean` puts it."""
    from gansynth_amd import _lib
    waves, table = STR.dense_table(lean=lean)
    total = STR.TOTAL
    assert total % 4 != 0 and 2 * _lib.MIX_TILE < total < 3 * _lib.MIX_TILE and len(table) == 40
    assert all(0 <= o < total and 1 <= h and 0 <= r and h + r <= STR.LENGTH for o, h, r, _, _, _ in table)
    assert any(o + h + r > total for o, h, r, _, _, _ in table)                     # a note is cut at the end
    ref, a, m = STR.mix(waves[:, :STR.LENGTH], table, total)
    assert 10 <= m.max() <= 16 and (m == 0).any()
    peaks = np.abs(ref).max(axis=1)
    assert peaks.min() > 1.0 and (peaks[1] > peaks[0]) == (lean > 0.5)
    err = np.abs(STR.mix_f32(waves[:, :STR.LENGTH], table, total).astype(np.float64) - ref)
    bound = SRF.bound(a, m[None])
    assert (err <= bound).all() and (err[a == 0] == 0).all()
    print(f"fp32 evaluation: worst error / bound = {(err[a > 0] / bound[a > 0]).max():.3f}, up to {m.max()} notes on a sample")


def test_finish_reference():
    x = np.array([[0.5, -2.0, 0.25], [1.5, 0.125, -0.75]], dtype=np.float32)
    peak, out, pcm = STR.finish(x, True)
    assert peak == 2.0 and out.tolist() == [[0.25, -1.0, 0.125], [0.75, 0.0625, -0.375]]
    assert pcm.shape == (3, 2) and pcm.tolist() == [[8192, 24576], [-32768, 2048], [4096, -12288]]
    peak, out, pcm = STR.finish(x, False)
    assert peak == 2.0 and np.array_equal(out, x) and pcm.tolist() == [[16384, 32767], [-32768, 4096], [8192, -24576]]
    peak, out, _ = STR.finish(x * 0.5, True)
    assert peak == 1.0 and np.array_equal(out, x * 0.5)                              # a peak of exactly 1 is left alone


# ---------------------------------------------------------------------------------------------------- driver and model
def test_driver_flags():
    import gan_synth_main as main
    args = main.parser.parse_args(["--synthesize", "score.mid"])
    assert (args.ensemble, args.stereo, args.spread) == (False, False, 0.0)
    assert (args.synthesize, args.output, args.seconds_per_instrument, args.release_seconds, args.seed, args.output_rate) == \
        ("score.mid", "synthesized.wav", 6.0, 1.0, 0, None)
    args = main.parser.parse_args(["--synthesize", "a.mid", "--ensemble", "--stereo", "--spread", "0.75"])
    assert (args.ensemble, args.stereo, args.spread) == (True, True, 0.75)
    assert main.parser.parse_args(["--stereo"]).ensemble is False and main.parser.parse_args(["--ensemble"]).stereo is False


def test_synthesize_signature():
    from gansynth_amd.models import GANSynth
    params = inspect.signature(GANSynth.synthesize).parameters
    assert (params["ensemble"].default, params["stereo"].default, params["spread"].default) == (False, False, 0.0)
    assert list(params)[-3:] == ["ensemble", "stereo", "spread"] and params["sample_rate"].default is None   # appended: positional calls keep their meaning
