"""CPU: the host layers of note sequences (DESIGN.md "Note sequences") -- the score reader on MIDI bytes assembled here, the schedule and
the latents against tests/synth_ref.py, the refusals of gs_note_mix (no launch), the table validation of kernels.note_mix and the
driver's flags."""
import ctypes
import json
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import synth_ref as SRF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ MIDI bytes
def vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.insert(0, (n & 0x7F) | 0x80)
        n >>= 7
    return bytes(out)


def track(events):
    body = b"".join(vlq(delta) + bytes(data) for delta, data in events)
    return b"MTrk" + struct.pack(">I", len(body)) + body


def header(fmt, ntracks, division):
    return b"MThd" + struct.pack(">IHHH", 6, fmt, ntracks, division)


def tempo(us):
    return [0xFF, 0x51, 0x03] + list(us.to_bytes(3, "big"))


END = [0xFF, 0x2F, 0x00]


def format0_file():
    """480 ticks per quarter, the default tempo (0.5 s per quarter) until tick 480, then 0.25 s per quarter."""
    return header(0, 1, 480) + track([
        (0, [0x90, 60, 100]),               # tick 0      0 s        A on
        (240, [62, 80]),                    # tick 240    0.25 s     B on, running status, a two-byte delta
        (240, [60, 0]),                     # tick 480    0.5 s      A off: note-on with velocity 0, running status
        (0, tempo(250000)),                 # tick 480               tempo change in mid-file
        (480, [0x80, 62, 64]),              # tick 960    0.75 s     B off
        (0, [0x99, 36, 127]),               # tick 960               channel 10: skipped
        (0, [0x90, 64, 70]),                # tick 960    0.75 s     C on
        (120, [64, 90]),                    # tick 1080   0.8125 s   the same pitch again: C ends, D begins
        (0, [0xF0, 0x03, 1, 2, 0xF7]),      #                        sysex, skipped by its length
        (60, [0x89, 36, 0]),                # tick 1140              channel 10 off
        (0, [0xFF, 0x01, 0x02, 0x68, 0x69]),  #                      a text meta event, skipped by its length
        (0, [0x90, 67, 32]),                # tick 1140   0.84375 s  E on, never ended
        (300, END),                         # tick 1440   1.0 s      the track's last event
    ])


def test_midi_format0():
    from gansynth_amd import notes as N
    got = N.read_notes(format0_file())
    want = [(60, 100, 0.0, 0.5), (62, 80, 0.25, 0.75), (64, 70, 0.75, 0.8125), (64, 90, 0.8125, 1.0), (67, 32, 0.84375, 1.0)]
    assert [(n.pitch, n.velocity) for n in got] == [w[:2] for w in want]
    for n, w in zip(got, want):
        assert abs(n.start - w[2]) <= 1e-9 and abs(n.end - w[3]) <= 1e-9, (n, w)
    assert all(isinstance(n, N.Note) for n in got)


def test_midi_format1_with_a_tempo_track(tmp_path):
    """96 ticks per quarter; the tempo track: 1 s per quarter, 0.5 s per quarter from tick 96; the notes are in the second track."""
    from gansynth_amd import notes as N
    data = header(1, 2, 96) + track([(0, tempo(1000000)), (96, tempo(500000)), (0, END)]) + \
        track([(0, [0x91, 48, 64]), (48, [0x90, 55, 1]), (144, [0x81, 48, 0]), (96, [0x80, 55, 0]), (0, END)])
    path = tmp_path / "two_tracks.mid"
    path.write_bytes(data)
    got = N.read_notes(str(path))
    assert [(n.pitch, n.velocity) for n in got] == [(48, 64), (55, 1)]
    want = [(0.0, 1.5), (0.5, 2.0)]   # tick 192 = 96 ticks at 1 s + 96 at 0.5 s; tick 48 = 0.5 s; tick 288 = 1 + 192 / 96 * 0.5
    for n, (s, e) in zip(got, want):
        assert abs(n.start - s) <= 1e-9 and abs(n.end - e) <= 1e-9, n


def test_midi_refusals():
    from gansynth_amd import notes as N
    body = track([(0, [0x90, 60, 100]), (10, [0x80, 60, 0]), (0, END)])
    with pytest.raises(ValueError, match="SMPTE"):
        N.read_notes(header(0, 1, 0xE728) + body)
    with pytest.raises(ValueError, match="format 2"):
        N.read_notes(header(2, 1, 96) + body)
    with pytest.raises(ValueError, match="truncated chunk"):
        N.read_notes(header(0, 1, 96) + body[:-3])
    with pytest.raises(ValueError, match="truncated"):      # the header announces a track that is not there
        N.read_notes(header(1, 2, 96) + body)
    cut = b"MTrk" + struct.pack(">I", 3) + bytes([0x00, 0x90, 60])   # the chunk ends inside an event
    with pytest.raises(ValueError, match="truncated track"):
        N.read_notes(header(0, 1, 96) + cut)


def test_json_scores(tmp_path):
    from gansynth_amd import notes as N
    items = [dict(pitch=60, velocity=100, start=0.5, end=1.0), dict(pitch=62, velocity=5, start=0.0, end=2.0),
             dict(pitch=64, velocity=127, start=0.5, end=0.75)]
    path = tmp_path / "score.json"
    path.write_text(json.dumps(items))
    got = N.read_notes(path)
    assert got == [N.Note(62, 5, 0.0, 2.0), N.Note(60, 100, 0.5, 1.0), N.Note(64, 127, 0.5, 0.75)]   # (start, order of appearance)
    assert N.read_notes(json.dumps(items).encode()) == got
    missing = [dict(items[0]), {k: v for k, v in items[1].items() if k != "velocity"}]
    with pytest.raises(ValueError, match=r"note 1 .*'velocity'"):
        N.read_notes(json.dumps(missing).encode())
    for field, value in (("pitch", "C4"), ("pitch", 60.5), ("velocity", 0), ("velocity", 128), ("start", -0.1), ("end", 0.5), ("start", None)):
        bad = [dict(items[0]), dict(items[2]), dict(items[0], **{field: value})]
        with pytest.raises(ValueError, match=rf"note 2 .*'{field}'"):
            N.read_notes(json.dumps(bad).encode())
    with pytest.raises(ValueError, match="JSON"):
        N.read_notes(b"\x00\x01 neither")


# -------------------------------------------------------------------------------------------------------------- schedule
def test_schedule_rounding_clamps_and_total():
    from gansynth_amd import notes as N
    sr, length = 16000, 1024
    notes = [N.Note(60, 127, 0.0, 0.5 / sr),                 # hold rounds 0.5 up to 1
             N.Note(61, 64, 10.4 / sr, 10.4 / sr + 0.2 / sr),  # onset 10, hold floor(0.7) = 0 -> clamped to 1
             N.Note(62, 1, 10.5 / sr, 10.5 / sr + 900.0 / sr),  # onset 11, hold 900, release cut to 124
             N.Note(63, 100, 0.01, 1.0),                      # onset 160, hold clamped to L, release 0
             N.Note(20, 100, 0.0, 1.0), N.Note(85, 100, 0.0, 1.0)]   # not in the table
    kept, table, total, dropped = N.schedule(notes, range(24, 85), sr, length, 0.01)
    assert dropped == 2 and [n.pitch for n in kept] == [60, 61, 62, 63]
    assert [row[:4] for row in table] == [(0, 1, 160, 0), (10, 1, 160, 1), (11, 900, 124, 2), (160, 1024, 0, 3)]
    assert [row[4] for row in table] == [1.0, 64 / 127, 1 / 127, 100 / 127]
    assert total == 160 + 1024
    ref_table, ref_total, ref_kept, ref_dropped = SRF.schedule([tuple(n) for n in notes], range(24, 85), sr, length, 0.01)
    assert ref_table == table and ref_total == total and ref_kept == [0, 1, 2, 3] and ref_dropped == dropped
    with pytest.raises(ValueError):
        N.schedule(notes[4:], range(24, 85), sr, length, 0.01)


def test_schedule_equals_the_restatement_on_the_dense_case():
    from gansynth_amd import notes as N
    _, notes = SRF.dense_case()
    kept, table, total, dropped = N.schedule([N.Note(*n) for n in notes], range(24, 85), SRF.SR, SRF.L, SRF.RELEASE / SRF.SR)
    ref_table, ref_total, ref_kept, _ = SRF.schedule(notes, range(24, 85), SRF.SR, SRF.L, SRF.RELEASE / SRF.SR)
    assert table == ref_table and total == ref_total and dropped == 0 and [tuple(n) for n in kept] == [notes[i] for i in ref_kept]
    labels = N.labels_for(kept, range(24, 85))
    assert labels.shape == (40, 61) and [int(r.argmax()) + 24 for r in labels] == [n.pitch for n in kept] and float(labels.sum()) == 40.0


def test_fp32_evaluation_sits_inside_the_bound():
    """The bound the kernel is held to, on the dense case of the GPU test: an fp32 evaluation in the stated order stays well inside it,
    and the draw has what it is meant to have (clamped holds, cut releases, many notes on one sample)."""
    waves, notes = SRF.dense_case()
    table, total, _, _ = SRF.schedule(notes, range(24, 85), SRF.SR, SRF.L, SRF.RELEASE / SRF.SR)
    assert sum(1 for _, h, _, _, _ in table if h == SRF.L) >= 5 and sum(1 for _, _, r, _, _ in table if r < SRF.RELEASE) >= 8
    ref, a, m = SRF.mix(waves, table, total)
    assert m.max() >= 8
    err = np.abs(SRF.mix_f32(waves, table, total).astype(np.float64) - ref)
    tight = (m + 4) * 2.0 ** -24 * a
    covered = a > 0
    assert (err <= tight).all() and (err[~covered] == 0).all()
    print(f"fp32 evaluation: worst error / ((M + 4) 2^-24 A) = {(err[covered] / tight[covered]).max():.3f}, up to {m.max()} notes on a sample")


def test_envelope():
    env = SRF.envelope(3, 4)
    assert env.tolist() == [1, 1, 1, 4 / 5, 3 / 5, 2 / 5, 1 / 5]     # would reach 1 at k = hold - 1 and 0 at k = hold + release
    assert SRF.envelope(2, 0).tolist() == [1, 1]


# ----------------------------------------------------------------------------------------------------- slerp and latents
def test_slerp():
    from gansynth_amd import notes as N
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(256), rng.standard_normal(256) * 3.0
    assert np.array_equal(N.slerp(a, b, 0.0), a) and np.array_equal(N.slerp(a, b, 1.0), b)
    assert np.array_equal(N.slerp(a, a, 0.3), a)                                       # the linear branch
    for t in (0.1, 0.5, 0.9):
        got = N.slerp(a, b, t)
        assert np.abs(got - SRF.slerp(a, b, t)).max() <= 1e-12
        coeff, residual, _, _ = np.linalg.lstsq(np.stack([a, b], axis=1), got, rcond=None)   # in the span of a and b
        assert np.abs(np.stack([a, b], axis=1) @ coeff - got).max() <= 1e-12 and (coeff > 0).all()
    u, v = a / np.linalg.norm(a), b / np.linalg.norm(b)
    assert abs(np.linalg.norm(N.slerp(u, v, 0.37)) - 1.0) <= 1e-12                  # unit vectors stay on the sphere


def test_latents_have_a_generator_of_their_own():
    from gansynth_amd import notes as N
    kept = [N.Note(60, 100, s, s + 0.5) for s in (0.0, 2.5, 6.0, 11.9, 13.0)]
    total = int(13.5 * 16000)
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    lat = N.schedule_latents(kept, total, 16000, 5, 6.0)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert lat.shape == (5, 256) and lat.dtype == torch.float32
    assert torch.equal(N.schedule_latents(kept, total, 16000, 5, 6.0), lat)
    assert not torch.equal(N.schedule_latents(kept, total, 16000, 6, 6.0), lat)
    k = int(13.5 // 6.0) + 1                                                           # anchors at 0, 6, 12, 18 s
    anchors = torch.randn(k + 1, 256, generator=torch.Generator().manual_seed(5)).double().numpy()
    assert torch.equal(lat[0], torch.from_numpy(anchors[0].astype(np.float32))) and torch.equal(lat[2], torch.from_numpy(anchors[1].astype(np.float32)))
    want = SRF.note_latents(anchors, [n.start for n in kept], 6.0)
    assert np.abs(lat.numpy() - want).max() <= 1e-6


# ---------------------------------------------------------------------------------------------------- ABI without a GPU
def test_note_mix_refusals_without_gpu():
    from gansynth_amd import _lib
    lib = _lib.load()
    P = 0x10000   # (never dereferenced: the argument checks come first and nothing is launched)
    good = dict(waves=P, rows=4, length=1024, row_stride=1024, notes=P, n_notes=3, total=5000, normalize=1, out=P, pcm=None, peak=None,
                ws=P, ws_bytes=1 << 20, stream=None)
    order = ["waves", "rows", "length", "row_stride", "notes", "n_notes", "total", "normalize", "out", "pcm", "peak", "ws", "ws_bytes", "stream"]
    bad = [("n_notes", 0, b"n_notes"), ("n_notes", -2, b"n_notes"), ("total", 0, b"total"), ("total", -1, b"total"), ("rows", 0, b"rows"),
           ("length", 0, b"length"), ("row_stride", 1023, b"row_stride"), ("waves", None, b"null"), ("notes", None, b"null"), ("out", None, b"null"),
           ("ws_bytes", 4, b"workspace"), ("ws", None, b"workspace")]
    for field, value, message in bad:
        args = dict(good, **{field: value})
        assert lib.gs_note_mix(*[args[k] for k in order]) == -1, (field, value)       # GS_ERR_ARG
        assert message in lib.gs_last_error(), (field, value, lib.gs_last_error())
    nbytes = lib.gs_note_mix_workspace_bytes
    assert nbytes(0) == 0 and nbytes(-5) == 0
    assert nbytes(1) == 4 and nbytes(_lib.MIX_TILE) == 4 and nbytes(_lib.MIX_TILE + 1) == 8 and nbytes(960000) == 4 * -(-960000 // _lib.MIX_TILE)
    assert nbytes(1 << 33) > nbytes(1 << 32)


def test_note_table_mirror_and_tile_constant():
    from gansynth_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gansynth_hip.h")).read()
    assert int(re.search(r"#define GS_MIX_TILE (\d+)", hdr).group(1)) == _lib.MIX_TILE
    assert ctypes.sizeof(_lib.GsMixNote) == 24
    assert [(n, getattr(_lib.GsMixNote, n).offset) for n, _ in _lib.GsMixNote._fields_] == \
        [("onset", 0), ("hold", 8), ("release", 12), ("row", 16), ("gain", 20)]


def test_note_mix_table_validation():
    from gansynth_amd import kernels
    good = [(100, 50, 10, 1, 0.5), (0, 64, 0, 0, 1.0), (100, 1, 63, 2, 0.25)]
    arr = kernels.note_mix_table(good, rows=3, length=64, total=200)
    assert [(n.onset, n.hold, n.release, n.row, n.gain) for n in arr] == [(0, 64, 0, 0, 1.0), (100, 50, 10, 1, 0.5), (100, 1, 63, 2, 0.25)]
    for field, value in (("onset", -1), ("onset", 200), ("hold", 0), ("hold", 65), ("release", -1), ("release", 15), ("row", 3), ("row", -1),
                         ("gain", float("nan")), ("hold", 2.5)):
        entry = dict(zip(("onset", "hold", "release", "row", "gain"), good[0]))
        entry[field] = value
        with pytest.raises(ValueError, match=rf"note 1 field '{field}'"):
            kernels.note_mix_table([good[1], tuple(entry.values()), good[2]], rows=3, length=64, total=200)
    with pytest.raises(ValueError):
        kernels.note_mix_table([], rows=3, length=64, total=200)


def test_driver_flags():
    import gan_synth_main as main
    args = main.parser.parse_args(["--synthesize", "score.mid"])
    assert (args.synthesize, args.output, args.seconds_per_instrument, args.release_seconds, args.seed) == ("score.mid", "synthesized.wav", 6.0, 1.0, 0)
    assert not (args.train or args.evaluate or args.generate or args.synthetic)
    args = main.parser.parse_args(["--synthesize", "a.json", "--output", "b.wav", "--seconds_per_instrument", "2.5", "--release_seconds", "0.25",
                                   "--seed", "9"])
    assert (args.synthesize, args.output, args.seconds_per_instrument, args.release_seconds, args.seed) == ("a.json", "b.wav", 2.5, 0.25, 9)
    assert main.parser.parse_args([]).synthesize is None
    args = main.parser.parse_args(["--synthesize", "score.txt"])
    with pytest.raises(SystemExit, match="mid"):
        main.synthesize_to_wav(None, args, range(24, 85))
