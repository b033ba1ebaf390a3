"""CPU: controllers (DESIGN.md "Controllers") -- notes.read_performance (the sustain pedal, the controller lists, the JSON object form),
notes.schedule_curves against tests/controllers_ref.py, kernels.note_mix_curves_table, the driver's flags, the library's refusals, and
the bound of tests/controllers_ref.py on the table that tests/test_controllers_gpu.py runs.  MIDI files are built here, as in
tests/test_ensemble_cpu.py (480 ticks per quarter at the default tempo: 960 ticks a second)."""
import ctypes
import inspect
import json
import math

import numpy as np
import pytest
import torch

from tests import controllers_ref as CRF
from tests import stereo_ref as STR
from tests.test_notes_cpu import END, header, tempo, track

T = 1 / 960   # one tick in seconds


def ends(performance):
    return [(n.pitch, round(n.end / T)) for n in performance.score.notes]


# ------------------------------------------------------------------------------------------------------------- the pedal
def pedal_file():
    """Format 1: a conductor, a track with the notes of channels 1 and 2, and a track that holds the pedal of channel 1 and the file's
    last event (tick 2000)."""
    conductor = track([(0, tempo(500000)), (0, END)])
    keys = track([
        (0, [0x90, 60, 100]),      # tick 0     A on
        (0, [0x91, 48, 90]),       #            X on, channel 2: no pedal there
        (200, [0x80, 60, 0]),      # tick 200   A off under the pedal (down at 100): held until the pedal-up at 500
        (0, [0x81, 48, 0]),        #            X off: stays
        (100, [0x90, 62, 100]),    # tick 300   B on
        (100, [0x80, 62, 0]),      # tick 400   B off under the pedal: held, but B comes again at 450
        (50, [0x90, 62, 80]),      # tick 450   B again
        (30, [0x80, 62, 0]),       # tick 480   off under the pedal: held until 500
        (120, [0x90, 64, 70]),     # tick 600   C on, the pedal is up
        (100, [0x80, 64, 0]),      # tick 700   C off: stays
        (200, [0x90, 65, 70]),     # tick 900   D on
        (100, [0x80, 65, 0]),      # tick 1000  D off under the second pedal, which never comes up: held to the file's last event
        (0, END)])
    feet = track([
        (100, [0xB0, 64, 127]),    # tick 100   down
        (400, [0xB0, 64, 0]),      # tick 500   up
        (300, [0xB0, 64, 64]),     # tick 800   down (64 is down)
        (1200, [0xB0, 11, 90]),    # tick 2000  the file's last event
        (0, END)])
    return header(1, 3, 480) + conductor + keys + feet


def test_pedal_in_a_midi_file():
    from gansynth_amd import notes as N
    data = pedal_file()
    perf = N.read_performance(data)
    plain = N.read_score(data)
    assert isinstance(perf, N.Performance) and isinstance(perf.score, N.Score)
    assert [(n.pitch, round(n.end / T)) for n in plain.notes] == [(60, 200), (48, 200), (62, 400), (62, 480), (64, 700), (65, 1000)]
    assert ends(perf) == [(60, 500), (48, 200), (62, 450), (62, 500), (64, 700), (65, 2000)]
    assert perf.pedal_extended == 4
    # everything but the ends is read_score's
    assert [n[:3] for n in perf.score.notes] == [n[:3] for n in plain.notes] and perf.score[1:] == plain[1:]
    # the reference's rule on the same ticks
    rows = [(0, 60, 0, 200), (1, 48, 0, 200), (0, 62, 300, 400), (0, 62, 450, 480), (0, 64, 600, 700), (0, 65, 900, 1000)]
    assert CRF.pedal(rows, {0: [(100, True), (500, False), (800, True)]}, 2000) == [500, 200, 450, 500, 700, 2000]
    # the expression event of channel 1 reaches its part, in seconds
    assert perf.controls == [[(2000 * T, "expression", 90)], []]


def test_pedal_ticks_pass_through_the_tempo_map():
    """The pedal is applied in ticks: with a tempo change between key-up and pedal-up the new end is the pedal-up's own time."""
    from gansynth_amd import notes as N
    data = header(0, 1, 480) + track([(0, [0xB0, 64, 100]), (0, [0x90, 60, 100]), (480, [0x80, 60, 0]), (0, tempo(250000)),
                                      (480, [0xB0, 64, 10]), (480, [0xB0, 7, 1]), (0, END)])
    perf = N.read_performance(data)
    assert perf.score.notes == [N.Note(60, 100, 0.0, 0.75)] and perf.pedal_extended == 1
    assert perf.controls == [[(1.0, "volume", 1)]]


def test_read_score_does_not_see_the_new_controllers():
    """A file full of CC 11 and CC 64: read_score and read_notes return what they return without them."""
    from gansynth_amd import notes as N
    data = header(0, 1, 480) + track([
        (0, [0xB0, 64, 127]), (0, [0xB0, 11, 5]), (0, [0xC0, 7]), (0, [0xB0, 7, 80]), (0, [0x90, 60, 100]), (10, [0xB0, 11, 60]),
        (230, [0x80, 60, 0]), (0, [0xB0, 64, 0]), (0, [0xB0, 10, 127]), (240, [0x90, 62, 50]), (0, [0xB0, 11, 127]), (480, [0x80, 62, 0]),
        (0, [0xB0, 64, 127]), (0, END)])
    want = N.Score([N.Note(60, 100, 0.0, 0.25), N.Note(62, 50, 0.5, 1.0)], [0, 0], [80, 80], [None, 1.0], [N.Part(0, 7)])
    assert N.read_score(data) == want and N.read_notes(data) == want.notes


# ------------------------------------------------------------------------------------------------------------ the curves
def _perf(N, controls, n_parts=None, pans=None):
    n_parts = len(controls) if n_parts is None else n_parts
    notes = [N.Note(60, 100, 0.0, 1.0) for _ in range(n_parts)]
    score = N.Score(notes, list(range(n_parts)), [100] * n_parts, pans or [None] * n_parts, [N.Part(None, None)] * n_parts)
    return N.Performance(score, controls, 0)


def _same(got, want):
    (points, first), (ref_points, ref_first) = got, want
    assert first == ref_first and len(points) == len(ref_points)
    for (pos, l, r), (ref_pos, ref_l, ref_r) in zip(points, ref_points):
        assert pos == ref_pos and np.float32(l) == ref_l and np.float32(r) == ref_r, (pos, l, r, ref_pos, ref_l, ref_r)


def test_curves_set_up_and_one_ramp():
    from gansynth_amd import notes as N
    sr = 16000
    # events on sample 0 (0.00003 s rounds to sample 0): one constant point, no fade-in
    perf = _perf(N, [[(0.0, "volume", 64), (0.00003, "expression", 100)]])
    points, first = N.schedule_curves(perf, [0], sr, 0.01, False, 0.0)
    a = np.float32((64 / 127) * (100 / 127))
    assert first == [0, 1] and points == [(0, float(a), float(a))]
    # no event at all: the defaults
    points, first = N.schedule_curves(_perf(N, [[]]), [0], sr, 0.01, False, 0.0)
    assert points == [(0, float(np.float32(100 / 127)), float(np.float32(100 / 127)))] and first == [0, 1]
    # one ramp: from the value at s to the target at s + R
    perf = _perf(N, [[(0.5, "expression", 0)]])
    points, first = N.schedule_curves(perf, [0], sr, 0.01, False, 0.0)
    v = float(np.float32(100 / 127))
    assert points == [(0, v, v), (8000, v, v), (8160, 0.0, 0.0)] and first == [0, 3]
    # a ramp of 0 seconds is one sample long
    assert N.schedule_curves(perf, [0], sr, 0.0, False, 0.0)[0][-1] == (8001, 0.0, 0.0)
    for bad in (-0.001, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="ramp"):
            N.schedule_curves(perf, [0], sr, bad, False, 0.0)
    for case in ([[(0.0, "volume", 64), (0.00003, "expression", 100)]], [[]], [[(0.5, "expression", 0)]]):
        _same(N.schedule_curves(_perf(N, case), [0], sr, 0.01, False, 0.0), CRF.curves(case, [0.0], sr, 0.01, False))


def test_curves_cut_collapse_and_targets():
    from gansynth_amd import notes as N
    sr = 16000
    # an event 80 samples into a 160-sample ramp cuts it at the float64 interpolation
    events = [(0.5, "expression", 0), (0.505, "expression", 127)]
    points, first = N.schedule_curves(_perf(N, [events]), [0], sr, 0.01, False, 0.0)
    v = 100 / 127
    cut = v + (8080 - 8000) / 160 * (0.0 - v)
    assert [p[0] for p in points] == [0, 8000, 8080, 8240] and points[2][1] == float(np.float32(cut)) and points[3][1] == float(np.float32(v))
    # the events of one sample collapse to the last state: no point for the first one
    same = [(0.25, "volume", 0), (0.25001, "volume", 127), (0.25002, "expression", 64)]
    points, _ = N.schedule_curves(_perf(N, [same]), [0], sr, 0.01, False, 0.0)
    assert [p[0] for p in points] == [0, 4000, 4160] and points[2][1] == float(np.float32(64 / 127))
    # mono: (a, a), pan events ignored; stereo: constant power, pan events count
    mixed = [(0.1, "pan", -1.0), (0.2, "volume", 127), (0.3, "pan", 0.5)]
    mono, _ = N.schedule_curves(_perf(N, [mixed]), [0], sr, 0.01, False, 0.0)
    assert [p[0] for p in mono] == [0, 3200, 3360] and all(l == r for _, l, r in mono)
    stereo, _ = N.schedule_curves(_perf(N, [mixed]), [0], sr, 0.01, True, 0.0)
    assert [p[0] for p in stereo] == [0, 1600, 1760, 3200, 3360, 4800, 4960]
    assert stereo[2][1:] == (float(np.float32(100 / 127)), float(np.float32(100 / 127 * math.sin(0.0))))         # hard left
    th = 1.5 * math.pi / 4
    assert stereo[-1][1:] == (float(np.float32(math.cos(th))), float(np.float32(math.sin(th))))
    # the default pan is the part's position: two free parts at spread 1 sit hard left and hard right; a panned part sits at 0
    spread, first = N.schedule_curves(_perf(N, [[], []]), [0, 1], sr, 0.01, True, 1.0)
    assert first == [0, 1, 2] and spread[0][2] == 0.0 and spread[1][1] == float(np.float32(100 / 127 * math.cos(math.pi / 2)))
    assert spread[0][1] == spread[1][2] == float(np.float32(100 / 127))
    panned, _ = N.schedule_curves(_perf(N, [[], []], pans=[0.3, None]), [0, 1], sr, 0.01, True, 1.0)
    assert panned[0][1] == panned[0][2] == panned[1][1] == panned[1][2] == float(np.float32(100 / 127 * math.cos(math.pi / 4)))
    # against the reference, several parts at once
    controls = [events, same, mixed, []]
    for stereo_on in (False, True):
        got = N.schedule_curves(_perf(N, controls), [0], sr, 0.003, stereo_on, 0.5)
        _same(got, CRF.curves(controls, N.part_positions(_perf(N, controls).score, 0.5), sr, 0.003, stereo_on))
        assert all(a[0] < b[0] for lo, hi in zip(got[1], got[1][1:]) for a, b in zip(got[0][lo:hi], got[0][lo + 1:hi]))
    with pytest.raises(ValueError, match="kept_index"):
        N.schedule_curves(_perf(N, [[]]), [1], sr, 0.01, False, 0.0)
    with pytest.raises(ValueError, match="spread"):
        N.schedule_curves(_perf(N, [[]]), [0], sr, 0.01, True, 2.0)


# ------------------------------------------------------------------------------------------------------- the JSON object
def _note(**more):
    return dict(dict(pitch=60, velocity=100, start=0.0, end=0.5), **more)


def test_json_performance():
    from gansynth_amd import notes as N
    plain = [_note(), _note(pitch=62, start=0.25, end=0.75, part=2, volume=90, pan=-0.5)]
    perf = N.read_performance(json.dumps(plain).encode())
    assert perf == N.Performance(N.read_score(json.dumps(plain).encode()), [[], []], 0)          # a list: no controls
    obj = {"notes": [_note(), _note(pitch=62, start=0.25, end=0.75, part=2), _note(start=0.625, end=0.7), _note(pitch=64, start=1.0, end=1.5)],
           "controls": [{"part": 2, "time": 0.5, "control": "pan", "value": -1},
                        {"part": 0, "time": 0.25, "control": "pedal", "value": True},
                        {"part": 0, "time": 0.125, "control": "volume", "value": 30},
                        {"part": 0, "time": 0.875, "control": "pedal", "value": 63},
                        {"part": 0, "time": 1.25, "control": "pedal", "value": 64},
                        {"part": 2, "time": 0.5, "control": "expression", "value": 5},
                        {"part": 0, "time": 3.0, "control": "expression", "value": 127}]}
    perf = N.read_performance(json.dumps(obj).encode())
    # pitch 60 of part 0 ends under the pedal: held to the re-trigger at 0.625; that one to the pedal-up at 0.875; the last to the last event
    assert [(n.pitch, n.start, n.end) for n in perf.score.notes] == [(60, 0.0, 0.625), (62, 0.25, 0.75), (60, 0.625, 0.875), (64, 1.0, 3.0)]
    assert perf.pedal_extended == 3 and perf.score.part == [0, 1, 0, 0] and perf.score.pan == [None] * 4
    assert perf.controls == [[(0.125, "volume", 30), (3.0, "expression", 127)], [(0.5, "pan", -1.0), (0.5, "expression", 5)]]
    assert N.control_counts(perf) == {"volume": 1, "expression": 2, "pan": 1}
    rows = [(0, 60, 0.0, 0.5), (1, 62, 0.25, 0.75), (0, 60, 0.625, 0.7), (0, 64, 1.0, 1.5)]
    assert CRF.pedal(rows, {0: [(0.25, True), (0.875, False), (1.25, True)]}, 3.0) == [0.625, 0.75, 0.875, 3.0]

    def refused(change, match):
        bad = json.loads(json.dumps(obj))
        change(bad)
        with pytest.raises(N.ScoreError, match=match):
            N.read_performance(json.dumps(bad).encode())

    refused(lambda o: o["notes"][1].update(volume=90), r"note 1 field 'volume'")
    refused(lambda o: o["notes"][2].update(pan=0.0), r"note 2 field 'pan'")
    refused(lambda o: o["notes"][3].pop("pitch"), r"note 3 has no field 'pitch'")
    refused(lambda o: o["controls"][0].update(part=1), r"control 0 field 'part'")
    refused(lambda o: o["controls"][1].update(part="0"), r"control 1 field 'part'")
    refused(lambda o: o["controls"][2].update(control="modulation"), r"control 2 field 'control'")
    refused(lambda o: o["controls"][2].update(value=128), r"control 2 field 'value'")
    refused(lambda o: o["controls"][2].update(value=1.5), r"control 2 field 'value'")
    refused(lambda o: o["controls"][0].update(value=1.01), r"control 0 field 'value'")
    refused(lambda o: o["controls"][3].update(value=-1), r"control 3 field 'value'")
    refused(lambda o: o["controls"][3].update(value="down"), r"control 3 field 'value'")
    refused(lambda o: o["controls"][5].update(time=-0.1), r"control 5 field 'time'")
    refused(lambda o: o["controls"][5].update(time="soon"), r"control 5 field 'time'")
    refused(lambda o: o["controls"][6].pop("value"), r"control 6 has no field 'value'")
    refused(lambda o: o["controls"].append(7), r"control 7 is not an object")
    refused(lambda o: o.update(controls={}), r"field 'controls'")
    refused(lambda o: o.update(tempo=120), r"unknown field 'tempo'")
    refused(lambda o: o.pop("notes"), r"no field 'notes'")
    with pytest.raises(N.ScoreError, match="list of note objects or an object"):
        N.read_performance(b"7")


# ------------------------------------------------------------------------------------------------------ the table and the library
def test_curve_mirrors():
    from gansynth_amd import _lib
    assert ctypes.sizeof(_lib.GsMixNoteCurve) == 32 and ctypes.sizeof(_lib.GsCurvePoint) == 16
    assert [(n, getattr(_lib.GsMixNoteCurve, n).offset) for n, _ in _lib.GsMixNoteCurve._fields_] == \
        [("onset", 0), ("hold", 8), ("release", 12), ("row", 16), ("gain", 20), ("curve", 24), ("reserved", 28)]
    assert [(n, getattr(_lib.GsCurvePoint, n).offset) for n, _ in _lib.GsCurvePoint._fields_] == [("pos", 0), ("v_l", 8), ("v_r", 12)]


def test_note_mix_curves_table_validation():
    from gansynth_amd import kernels
    good = [(100, 50, 10, 1, 0.5, 1), (0, 64, 0, 0, 1.0, 0), (100, 1, 63, 2, 0.25, 0)]
    points, first = [(0, 1.0, 0.5), (10, 0.5, 0.25), (5, 0.125, 1.0)], [0, 2, 3]
    notes, pts, firsts = kernels.note_mix_curves_table(good, points, first, rows=3, length=64, total=200)
    assert [(n.onset, n.hold, n.release, n.row, n.gain, n.curve, n.reserved) for n in notes] == \
        [(0, 64, 0, 0, 1.0, 0, 0), (100, 50, 10, 1, 0.5, 1, 0), (100, 1, 63, 2, 0.25, 0, 0)]
    assert [(p.pos, p.v_l, p.v_r) for p in pts] == points and list(firsts) == first

    def refused(match, table=good, points=points, first=first):
        with pytest.raises(ValueError, match=match):
            kernels.note_mix_curves_table(table, points, first, rows=3, length=64, total=200)

    for field, value in (("onset", -1), ("onset", 200), ("hold", 0), ("hold", 65), ("release", -1), ("release", 15), ("row", 3), ("row", -1),
                         ("gain", float("nan")), ("gain", None), ("gain", True), ("hold", 2.5), ("curve", 2), ("curve", -1), ("curve", 0.0),
                         ("curve", True)):
        entry = dict(zip(("onset", "hold", "release", "row", "gain", "curve"), good[0]))
        entry[field] = value
        refused(rf"note_mix_curves: note 1 field '{field}'", table=[good[1], tuple(entry.values()), good[2]])
    refused("empty", table=[])
    refused("note 0 has 5 fields", table=[(0, 64, 0, 0, 1.0)])
    refused("first must run from 0", first=[1, 2, 3])
    refused("first must run from 0", first=[0, 2, 4])
    refused("first must run from 0", first=[0])
    refused("curve 1 has no point", first=[0, 2, 2, 3])
    refused("curve 1 has no point", first=[0, 3, 2, 3])                                                    # decreasing
    refused(r"first\[1\] must be an integer", first=[0, 2.0, 3])
    refused("point 1 field 'pos'", points=[(0, 1.0, 0.5), (0, 0.5, 0.25), (5, 0.125, 1.0)])                 # not increasing inside curve 0
    refused("point 1 field 'pos'", points=[(0, 1.0, 0.5), (1.5, 0.5, 0.25), (5, 0.125, 1.0)])
    refused("point 2 field 'v_r'", points=[(0, 1.0, 0.5), (10, 0.5, 0.25), (5, 0.125, float("inf"))])
    refused("point 0 field 'v_l'", points=[(0, float("nan"), 0.5), (10, 0.5, 0.25), (5, 0.125, 1.0)])
    refused("point 0 has 2 fields", points=[(0, 1.0), (10, 0.5, 0.25), (5, 0.125, 1.0)])


def test_note_mix_curves_validates_before_the_library_call():
    from gansynth_amd import kernels

    class Lib:
        def __getattr__(self, name):
            raise AssertionError(f"{name} reached")

    K = kernels.HipKernels.__new__(kernels.HipKernels)
    K.lib = Lib()
    waves = torch.zeros(3, 64)
    with pytest.raises(ValueError, match=r"note 0 field 'curve'"):
        K.note_mix_curves(waves, [(0, 64, 0, 0, 1.0, 1)], [(0, 1.0, 1.0)], [0, 1], 200)
    with pytest.raises(ValueError, match="channels must be 1 or 2"):
        K.note_mix_curves(waves, [(0, 64, 0, 0, 1.0, 0)], [(0, 1.0, 1.0)], [0, 1], 200, channels=3)
    with pytest.raises(ValueError, match="waves must be"):
        K.note_mix_curves(waves.double(), [(0, 64, 0, 0, 1.0, 0)], [(0, 1.0, 1.0)], [0, 1], 200)
    with pytest.raises(AssertionError, match="gs_note_mix_curves_workspace_bytes reached"):
        K.note_mix_curves(waves, [(0, 64, 0, 0, 1.0, 0)], [(0, 1.0, 1.0)], [0, 1], 200)


REFUSALS = [("n_notes", 0, b"n_notes"), ("total", 0, b"total"), ("rows", 0, b"rows"), ("length", -1, b"length"), ("row_stride", 1023, b"row_stride"),
            ("out_stride", 4999, b"out_stride"), ("waves", None, b"null"), ("notes", None, b"null"), ("out", None, b"null"),
            ("notes", 0x10004, b"notes must be 8-byte"), ("pcm", 0x10001, b"pcm must be 2-byte"), ("out", 0x10002, b"4-byte"),
            ("ws_bytes", 4, b"workspace"), ("ws", None, b"workspace"), ("n_points", 0, b"n_points"), ("n_points", -1, b"n_points"),
            ("n_curves", 0, b"n_curves"), ("channels", 0, b"channels"), ("channels", 3, b"channels"), ("points", None, b"null"),
            ("first", None, b"null"), ("points", 0x10004, b"points must be 8-byte"), ("first", 0x10002, b"first must be 4-byte")]


def curves_args(**change):
    P = 0x10000   # (never dereferenced: the argument checks come first and nothing is launched)
    good = dict(waves=P, rows=4, length=1024, row_stride=1024, notes=P, n_notes=3, points=P, n_points=5, first=P, n_curves=2, channels=2,
                total=5000, normalize=1, out=P, out_stride=5000, pcm=None, peak=None, ws=P, ws_bytes=1 << 20, stream=None)
    return list(dict(good, **change).values())


def test_note_mix_curves_refusals_without_gpu():
    from gansynth_amd import _lib
    lib = _lib.load()
    for field, value, message in REFUSALS:
        assert lib.gs_note_mix_curves(*curves_args(**{field: value})) == -1, (field, value)       # GS_ERR_ARG
        assert message in lib.gs_last_error() and b"note_mix_curves" in lib.gs_last_error(), (field, value, lib.gs_last_error())
    nbytes = lib.gs_note_mix_curves_workspace_bytes
    assert nbytes(0) == 0 and nbytes(-5) == 0 and nbytes(1) == 4 and nbytes(_lib.MIX_TILE + 1) == 8


# -------------------------------------------------------------------------------------------------------- driver and model
def test_controller_flags():
    import gan_synth_main as main
    args = main.parser.parse_args(["--synthesize", "score.mid"])
    assert (args.controllers, args.controller_ramp) == (False, 0.01) and main.check_controller_args(args) is False
    args = main.parser.parse_args(["--synthesize", "a.mid", "--controllers", "--controller_ramp", "0.05"])
    assert (args.controllers, args.controller_ramp) == (True, 0.05) and main.check_controller_args(args) is True
    assert main.check_controller_args(main.parser.parse_args(["--synthesize", "a.mid", "--controllers", "--controller_ramp", "0"])) is True
    for argv, message in ((["--synthesize", "a.mid", "--controller_ramp", "0.02"], "needs --controllers"),
                          (["--controllers"], "--synthesize only"),
                          (["--synthesize", "a.mid", "--controllers", "--controller_ramp", "-0.01"], "non-negative"),
                          (["--synthesize", "a.mid", "--controllers", "--controller_ramp", "nan"], "non-negative"),
                          (["--synthesize", "a.mid", "--controllers", "--controller_ramp", "inf"], "finite")):
        with pytest.raises(SystemExit, match=message):
            main.check_controller_args(main.parser.parse_args(argv))


def test_synthesize_takes_controllers():
    from gansynth_amd.models import GANSynth
    params = inspect.signature(GANSynth.synthesize).parameters
    assert (params["controllers"].default, params["controller_ramp"].default) == (False, 0.01)


# ------------------------------------------------------------------------------------ the bound, on the GPU test's table
@pytest.mark.parametrize("channels", [1, 2])
def test_fp32_evaluation_sits_inside_the_bound(channels):
    """The table and curves of tests/test_controllers_gpu.py: an fp32 evaluation in the stated order stays inside (M + 12) 2^-24 A, and
    the case has what it is meant to have."""
    from gansynth_amd import _lib
    waves, table, points, first = CRF.dense_case()
    total, tile = STR.TOTAL, _lib.MIX_TILE
    assert len(table) == 40 and len(first) == 6 and {row[5] for row in table} == {0, 1, 2, 3, 4}
    order = sorted(range(40), key=lambda i: (table[i][0], i))
    assert sum(table[a][5] != table[b][5] for a, b in zip(order, order[1:])) >= 30          # neighbouring candidates change part
    pos = [[p[0] for p in points[lo:hi]] for lo, hi in zip(first, first[1:])]
    assert {tile - 1, tile, tile + 1} <= set(pos[0]) and {4200, 4201, 4202, 4203} <= set(pos[0]) and 4200 % 4 == 0
    assert pos[1][0] < tile and pos[1][1] > 2 * tile and len(pos[2]) == 1
    assert pos[3][0] > min(row[0] for row in table) and pos[3][-1] < total and any(p[1] == 0.0 for p in points[first[4]:first[5]])
    assert all(p[1] >= 0 and p[2] >= 0 for p in points)                                     # what the bound's derivation asks
    ref, a, m = CRF.mix(waves[:, :STR.LENGTH], table, points, first, total, channels)
    got = CRF.mix_f32(waves[:, :STR.LENGTH], table, points, first, total, channels)
    err = np.abs(got.astype(np.float64) - ref)
    bound = CRF.bound(a, m[None])
    assert (err <= bound).all() and (got[a == 0] == 0).all() and m.max() >= 10
    print(f"fp32 evaluation, {channels} channel(s): worst error / bound = {(err[a > 0] / bound[a > 0]).max():.3f}")
    # constant curves of 1: the stated order gives tests/stereo_ref.py's sums bit for bit
    ones, one_first = [(0, 1.0, 1.0)] * 5, [0, 1, 2, 3, 4, 5]
    plain = STR.mix_f32(waves[:, :STR.LENGTH], [row[:5] + (row[4],) for row in table], total)
    assert np.array_equal(CRF.mix_f32(waves[:, :STR.LENGTH], table, ones, one_first, total, channels), plain[:channels])
