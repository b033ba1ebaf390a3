"""No GPU: pitch bend on the host (DESIGN.md "Pitch bend") -- the reader (MIDI bend and RPN 0,0, JSON "bend" controls), notes.schedule_bends
against tests/bend_ref.py and a brute-force integral, the library's coefficient table bit for bit, the quality of the float64 rule on
sines, the fp32 restatement against the float64 rule on the GPU test's inputs, the host checks of kernels.note_warp_table and the
entry point's refusals."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

from tests import bend_ref as B
from tests.test_notes_cpu import END, header, track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rpn(status, msb, lsb):
    return [(0, [status, 101, msb]), (0, [status, 100, lsb])]


def bend(value):
    v = value + 8192
    return [v & 0x7F, v >> 7]


# ---------------------------------------------------------------------------------------------------------------- reader
def bend_file():
    """Format 1, 480 ticks a quarter at the default tempo (960 ticks a second).  Channel 1 bends under the default range, then sets 12
    semitones and 50 cents through RPN 0,0 (data entry under running status), deselects, and a later CC 6 must not count; channel 2
    (program 33) asks for 40 semitones and gets 24; channel 10 bends and is ignored."""
    one = track([
        (0, [0x90, 60, 100]),
        (96, [0xE0] + bend(4096)),          # tick 96    +1 semitone of the default 2
        (96, bend(-8192)),                  # tick 192   running status: -2
        (48, [0xB0, 101, 0]),               # tick 240   RPN 0,0 ...
        (0, [100, 0]),                      #            ... under running status
        (0, [6, 12]),                       #            range 12: a new target from the value in force, -12
        (0, [38, 50]),                      #            and 50 cents: -12.5
        (0, [101, 127]), (0, [100, 127]),   #            deselected
        (48, [6, 3]),                       # tick 288   data entry for nothing: no event
        (0, [0xE0] + bend(8191)),           #            +8191 / 8192 * 12.5
        (192, [0x80, 60, 0]),               # tick 480
        (0, END)])
    two = track([
        (0, [0xC1, 33]),
        *rpn(0xB1, 0, 0), (0, [0xB1, 6, 40]),          # tick 0     range 40 -> 24, target 0
        (10, [0x91, 48, 80]),
        (86, [0xE1] + bend(-4096)),                    # tick 96    -12
        (0, [0xE9] + bend(8191)),                      #            channel 10: ignored
        (0, [0xB9, 101, 0]), (0, [0xB9, 100, 0]), (0, [0xB9, 6, 5]),
        (100, [0x81, 48, 0]),
        (0, END)])
    return header(1, 2, 480) + one + two


def test_midi_bend_and_rpn():
    from gansynth_amd import notes as N
    data = bend_file()
    bends = N.read_bends(data)
    score = N.read_score(data)
    assert score.parts == [N.Part(0, 0), N.Part(1, 33)] and len(bends) == 2
    at = lambda tick: tick * 500000 / (480 * 1e6)
    assert bends[0] == [(at(96), 4096 / 8192 * 2.0), (at(192), -2.0), (at(240), -12.0), (at(240), -12.5), (at(288), 8191 / 8192 * 12.5)]
    assert bends[1] == [(at(0), 0.0), (at(96), -12.0)]
    # the other readers are deaf to all of it, as they were
    assert N.read_performance(data).controls == [[], []] and N.read_notes(data) == score.notes


def test_json_bend(tmp_path):
    from gansynth_amd import notes as N
    notes = [{"pitch": 60, "velocity": 100, "start": 0.0, "end": 0.5, "part": 3}, {"pitch": 64, "velocity": 90, "start": 0.1, "end": 0.4, "part": 1}]
    obj = {"notes": notes, "controls": [{"part": 3, "time": 0.2, "control": "bend", "value": -1.5},
                                        {"part": 1, "time": 0.0, "control": "volume", "value": 90},
                                        {"part": 3, "time": 0.1, "control": "bend", "value": 24},
                                        {"part": 1, "time": 0.3, "control": "bend", "value": 0}]}
    path = tmp_path / "s.json"
    path.write_text(json.dumps(obj))
    assert N.read_bends(str(path)) == [[(0.3, 0.0)], [(0.1, 24.0), (0.2, -1.5)]]           # parts in ascending order of "part": 1, then 3
    performance = N.read_performance(str(path))
    assert performance.controls == [[(0.0, "volume", 90)], []] and N.control_counts(performance) == {"volume": 1, "expression": 0, "pan": 0}
    assert N.read_bends(json.dumps(notes).encode()) == [[], []]
    for value in (24.5, -25, "1", None, True, float("nan")):
        bad = {"notes": notes, "controls": [{"part": 1, "time": 0.0, "control": "volume", "value": 1}, {"part": 3, "time": 0.0, "control": "bend", "value": value}]}
        with pytest.raises(N.ScoreError, match="control 1 field 'value' must be a number of semitones in \\[-24, 24\\] for 'bend'"):
            N.read_bends(json.dumps(bad).encode())
    with pytest.raises(N.ScoreError, match="control 0 field 'part'"):
        N.read_bends(json.dumps({"notes": notes, "controls": [{"part": 2, "time": 0.0, "control": "bend", "value": 1}]}).encode())
    with pytest.raises(N.ScoreError, match="control 0 field 'time'"):
        N.read_bends(json.dumps({"notes": notes, "controls": [{"part": 1, "time": -1, "control": "bend", "value": 1}]}).encode())
    with pytest.raises(N.ScoreError, match="control 0 has no field 'value'"):
        N.read_bends(json.dumps({"notes": notes, "controls": [{"part": 1, "time": 0, "control": "bend"}]}).encode())
    with pytest.raises(N.ScoreError, match="control 0 field 'control'"):
        N.read_bends(json.dumps({"notes": notes, "controls": [{"part": 1, "time": 0, "control": "wheel", "value": 1}]}).encode())


def test_existing_scores_read_as_before():
    """A controllers MIDI file and a controllers JSON through read_performance: what they gave before bends were read."""
    from gansynth_amd import notes as N
    from tests.test_controllers_gpu import _performance_file
    at = lambda tick: tick * 500000 / (480 * 1e6)
    performance = N.read_performance(_performance_file())
    assert performance.controls == [[(0.0, "volume", 110), (at(20), "expression", 40), (at(32), "expression", 120)],
                                    [(0.0, "pan", (20 - 64) / 63), (at(25), "pan", (110 - 64) / 63), (at(95), "volume", 60)]]
    assert performance.pedal_extended == 1 and N.read_bends(_performance_file()) == [[], []]
    assert set(N._CONTROLLERS.items()) == {(7, "volume"), (10, "pan"), (11, "expression"), (64, "pedal")}
    assert N.CONTROL_KINDS == ("volume", "expression", "pan")
    obj = {"notes": [{"pitch": 60, "velocity": 100, "start": 0.0, "end": 0.2}],
           "controls": [{"part": 0, "time": 0.1, "control": "expression", "value": 64}, {"part": 0, "time": 0.15, "control": "pedal", "value": True},
                        {"part": 0, "time": 0.4, "control": "pedal", "value": 0}]}
    got = N.read_performance(json.dumps(obj).encode())
    assert got.controls == [[(0.1, "expression", 64)]] and got.pedal_extended == 1 and got.score.notes[0].end == 0.4


# -------------------------------------------------------------------------------------------------------- schedule_bends
def test_schedule_bends_conventions():
    from gansynth_amd import notes as N
    sr = 16000
    # set-up at sample 0: the value, no ramp; a part without an event: no curve
    points, first = N.schedule_bends([[(0.0, 1.0), (0.00001, 2.0)], [], [(0.0, 0.0)]], sr, 0.01)
    assert first == [0, 1, 1, 2] and points == [(0.0, 2.0 ** (2 / 12), 0.0), (0.0, 1.0, 0.0)]
    # a later event: a ramp in semitones of R = 160 samples from the value there
    points, first = N.schedule_bends([[(0.1, 2.0)]], sr, 0.01)
    assert [(p, r) for p, r, _ in points] == [(0.0, 1.0), (1600.0, 1.0), (1760.0, 2.0 ** (2 / 12))] and points[1][2] == 1600.0
    # a ramp in progress is cut at its interpolated value: at sample 1680 the first ramp stands at 1 semitone
    points, _ = N.schedule_bends([[(0.1, 2.0), (0.105, 0.0)]], sr, 0.01)
    assert [(p, r) for p, r, _ in points] == [(0.0, 1.0), (1600.0, 1.0), (1680.0, 2.0 ** (1 / 12)), (1840.0, 1.0)]
    # a ramp longer than 160 samples is cut into pieces of at most 160, linear in semitones
    points, _ = N.schedule_bends([[(0.1, 4.0)]], sr, 0.025)
    assert [(p, r) for p, r, _ in points] == [(0.0, 1.0), (1600.0, 1.0), (1760.0, 2.0 ** (1.6 / 12)), (1920.0, 2.0 ** (3.2 / 12)), (2000.0, 2.0 ** (4 / 12))]
    # the clamp of the ratio
    points, _ = N.schedule_bends([[(0.0, 36.0)], [(0.0, -36.0)]], sr, 0.01)
    assert [r for _, r, _ in points] == [4.0, 0.25]
    # the restatement agrees on a busier part, bit for bit
    events = [[(0.0, -1.0), (0.03, 2.0), (0.031, 2.5), (0.2, -7.0), (0.2, 0.5), (0.2001, 1.0)], [], [(0.5, 12.0), (0.52, -12.0)]]
    assert N.schedule_bends(events, sr, 0.04) == B.curves(events, sr, 0.04)
    for ramp in (-0.01, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="schedule_bends: ramp_seconds"):
            N.schedule_bends(events, sr, ramp)
    with pytest.raises(ValueError, match="schedule_bends: part 1 holds"):
        N.schedule_bends([[], [(0.1, float("nan"))]], sr, 0.01)


def test_cum_against_a_riemann_sum():
    """cum = Phi(pos): against a brute-force float64 midpoint sum of the ratio (linear between points) at 1/64 of a sample."""
    from gansynth_amd import notes as N
    events = [[(0.0, 1.0), (0.01, 3.0), (0.05, -5.0), (0.055, 0.0)]]
    points, _ = N.schedule_bends(events, 16000, 0.02)
    pos, ratio, cum = (np.array(v) for v in zip(*points))
    s = (np.arange(int(pos[-1]) * 64) + 0.5) / 64.0
    brute = np.concatenate([[0.0], np.cumsum(np.interp(s, pos, ratio)) / 64.0])
    want = brute[(pos * 64).astype(np.int64)]
    assert np.abs(cum - want).max() <= 1e-9 * pos[-1]                       # (the midpoint rule is exact on linear pieces: rounding only)
    # and Phi between the points, through the restatement's evaluation
    t = np.arange(int(pos[-1]) + 50, dtype=np.float64)
    got, r = B.phi(points, t)
    inside = t <= pos[-1]
    assert np.abs(got[inside] - brute[(t[inside] * 64).astype(np.int64)]).max() <= 1e-9 * pos[-1]
    assert np.array_equal(r[~inside], np.full((~inside).sum(), ratio[-1])) and np.allclose(got[~inside], cum[-1] + ratio[-1] * (t[~inside] - pos[-1]))


def test_bent_notes():
    from gansynth_amd import notes as N
    points, first = N.schedule_bends([[(0.1, 2.0), (0.2, 0.0)], [], [(0.0, 0.0)]], 16000, 0.01)     # part 0 leaves 1 in (1600, 3360): samples 1601 .. 3359
    table = [(0, 1000, 601, 0, 1.0), (0, 1000, 602, 1, 1.0), (1700, 10, 0, 2, 1.0), (3360, 100, 0, 3, 1.0), (3359, 1, 0, 4, 1.0), (1700, 10, 0, 5, 1.0),
             (1700, 10, 0, 6, 1.0)]
    assert N.bent_notes(table, [0, 0, 0, 0, 0, 1, 2], points, first) == [1, 2, 4]


# ----------------------------------------------------------------------------------------------------------------- table
def test_table_bit_for_bit():
    from gansynth_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "gansynth_hip.h")).read()
    floats = int(re.search(r"#define GS_WARP_TABLE_FLOATS (\d+)", hdr).group(1))
    assert lib.gs_note_warp_table_bytes() == 4 * floats and floats >= B.ZQ + 2 and floats % 4 == 0
    assert (int(re.search(r"#define GS_WARP_TILE (\d+)", hdr).group(1)), int(re.search(r"#define GS_WARP_ZEROS (\d+)", hdr).group(1)),
            int(re.search(r"#define GS_WARP_Q (\d+)", hdr).group(1))) == (_lib.WARP_TILE, _lib.WARP_ZEROS, _lib.WARP_Q) == (B.TILE, B.Z, B.Q)
    host = np.full(floats, np.nan, dtype=np.float32)
    assert lib.gs_note_warp_table(host.ctypes.data) == 0
    want = B.table()
    assert np.array_equal(host[:B.ZQ + 2].view(np.uint32), want.view(np.uint32)) and (host[B.ZQ + 1:] == 0).all()
    assert host[0] == 1.0 and (host[B.Q:B.ZQ + 1:B.Q] == 0).all() and np.count_nonzero(host[:B.ZQ] == 0) == B.Z - 1
    assert lib.gs_note_warp_table(None) == -1 and b"note_warp_table" in lib.gs_last_error()


def test_struct_mirrors():
    from gansynth_amd import _lib
    assert ctypes.sizeof(_lib.GsWarpNote) == 24 and ctypes.sizeof(_lib.GsWarpPoint) == 24
    assert [(n, getattr(_lib.GsWarpNote, n).offset) for n, _ in _lib.GsWarpNote._fields_] == \
        [("src_row", 0), ("dst_row", 4), ("onset", 8), ("count", 16), ("curve", 20)]
    assert [(n, getattr(_lib.GsWarpPoint, n).offset) for n, _ in _lib.GsWarpPoint._fields_] == [("pos", 0), ("ratio", 8), ("cum", 16)]


# --------------------------------------------------------------------------------------------- quality of the float64 rule
# Measured with this file's functions (DESIGN.md "Pitch bend" holds the table); each bound is twice the worst figure, rounded up to one
# digit -- the 2 allows for the few frequencies sampled.
L = 4096
FREQS = (0.05, 0.25, 0.45, 0.65, 0.85)        # of Nyquist
PASSBAND_BOUND, IMAGE_BOUND, PEAK_BOUND = 3e-5, 8e-7, 5e-5      # measured: 1.35e-5, 3.74e-7, 2.27e-5


def _interior(ratio, count):
    return slice(int(130 / ratio) + 2, count - 2)     # outputs whose taps all lie inside the row


def test_constant_ratio_against_the_analytic_sine():
    """A sine at f of the LOWER of the two Nyquist frequencies (so that it lies in the passband at every ratio) under a constant ratio r
    is the sine of r times the frequency."""
    worst = 0.0
    for r in (0.25, 0.5, 2.0 ** (-2 / 12), 2.0 ** (1 / 12), 2.0 ** (2 / 12), 2.0, 4.0):
        count = min(L, int((L - 300) / r))
        for f in FREQS:
            fin = f / max(1.0, r)
            x = np.sin(np.pi * fin * np.arange(L)).astype(np.float32)
            y = B.warp_note(x, [(0.0, r, 0.0)], 0, count)
            err = np.abs(y - np.sin(np.pi * fin * r * np.arange(count)))[_interior(r, count)].max()
            print(f"ratio {r:.4f}, {f} of Nyquist: {err:.3g}")
            worst = max(worst, err)
    assert worst <= PASSBAND_BOUND, worst


def test_images_above_the_new_nyquist():
    """A sine above the cutoff 1 / r of the input band (by 15 % and more: beyond the transition band) must vanish, not alias."""
    worst = 0.0
    for r in (2.0, 4.0):
        count = int((L - 300) / r)
        for f in (f for f in FREQS if f >= 1.15 / r):
            x = np.sin(np.pi * f * np.arange(L)).astype(np.float32)
            level = np.abs(B.warp_note(x, [(0.0, r, 0.0)], 0, count))[_interior(r, count)].max()
            print(f"ratio {r}, {f} of Nyquist: {level:.3g}")
            worst = max(worst, level)
    assert worst <= IMAGE_BOUND, worst


def test_a_bent_sine_lands_at_f_times_the_ratio():
    points, _ = B.curves([[(0.01, 2.0)]], 16000, 0.01)          # up two semitones over samples 160 .. 320
    ratio, worst = 2.0 ** (2 / 12), 0.0
    for f in (f for f in FREQS if f * ratio < 0.9):
        x = np.sin(np.pi * f * np.arange(L)).astype(np.float32)
        y = B.warp_note(x, points, 0, 3000)
        spectrum = np.abs(np.fft.rfft(y[600:600 + 2048] * np.hanning(2048), 1 << 18))
        got = np.argmax(spectrum) / (1 << 17)
        print(f"{f} of Nyquist: peak at {got:.6f}, {f * ratio:.6f} expected")
        worst = max(worst, abs(got - f * ratio) / (f * ratio))
    assert worst <= PEAK_BOUND, worst


# ------------------------------------------------------------------------------------------------------- fp32 restatement
def test_fp32_restatement_on_the_gpu_cases():
    """warp_f32 against warp_f64 on the inputs of tests/test_bend_gpu.py: e = max |z - y64| / max B per case.  fp32 sums of up to 256
    rounded products of rounded coefficients: a few 2^-24; an exact 0 where the ratio is 1 or a single first sample is copied.  The GPU
    test allows the kernel four times these figures."""
    x = B.source()
    for name, case in B.cases().items():
        results = B.run_case(x, case, "f32")
        z, y64, bound = (np.concatenate([r[i] for r in results]) for i in range(3))
        e = B.error_ratio(z, y64, bound)
        print(f"{name}: e(warp_f32) = {e:.3g} = {e * 2 ** 24:.2f} * 2^-24, max B = {bound.max():.3g}")
        # the a-priori bound of a sum of 2 HALF products one after the other, each coefficient five roundings from its operands
        assert np.isfinite(z).all() and e <= (2 * B.HALF + 5) * 2.0 ** -24, (name, e)
        if name in ("ratio 1", "count 1"):
            assert e == 0.0 and np.array_equal(z, x[:len(z)])
    # a note bent up runs out of waveform and ends in exact zeros
    (z, y64, _), = B.run_case(x, B.cases()["ratio 4"], "f32")
    assert (z[-2000:] == 0).all() and (y64[-2000:] == 0).all() and np.abs(z[:700]).max() > 0.1


# ---------------------------------------------------------------------------------------------- host checks and refusals
GOOD_NOTES = [(0, 2, 0, 100, 0), (1, 3, 5, 1024, 1)]
GOOD_POINTS, GOOD_FIRST = [(0.0, 1.0, 0.0), (10.0, 1.5, 12.5), (0.0, 0.5, 0.0)], [0, 2, 3]
BAD_NOTES = [((-1, 2, 0, 100, 0), "note 0 field 'src_row'"), ((4, 2, 0, 100, 0), "note 0 field 'src_row'"), ((0, 4, 0, 100, 0), "note 0 field 'dst_row'"),
             ((0, -1, 0, 100, 0), "note 0 field 'dst_row'"), ((0, 0, 0, 100, 0), "note 0 field 'dst_row'"), ((0, 1, 0, 100, 0), "note 0 field 'dst_row'"),
             ((0, 3, 0, 100, 0), "note 1 field 'dst_row'"), ((0, 2, 0, 0, 0), "note 0 field 'count'"), ((0, 2, 0, 1025, 0), "note 0 field 'count'"),
             ((0, 2, -1, 100, 0), "note 0 field 'onset'"), ((0, 2, 0, 100, 2), "note 0 field 'curve'"), ((0, 2, 0, 100, -1), "note 0 field 'curve'"),
             ((0, 2, 0.5, 100, 0), "note 0 field 'onset'"), ((0, 2, 0, 100), "note 0 has 4 fields")]


def test_note_warp_table_validation():
    from gansynth_amd import kernels
    notes, points, first = kernels.note_warp_table(GOOD_NOTES, GOOD_POINTS, GOOD_FIRST, 4, 1024)
    assert (notes[1].src_row, notes[1].dst_row, notes[1].onset, notes[1].count, notes[1].curve) == (1, 3, 5, 1024, 1)
    assert (points[1].pos, points[1].ratio, points[1].cum) == (10.0, 1.5, 12.5) and list(first) == [0, 2, 3]
    for bad, message in BAD_NOTES:
        with pytest.raises(ValueError, match="note_warp: " + message):
            kernels.note_warp_table([bad, GOOD_NOTES[1]], GOOD_POINTS, GOOD_FIRST, 4, 1024)
    for bad, message in (([(0.0, 1.0, 0.0), (0.0, 1.5, 12.5), (0.0, 0.5, 0.0)], "point 1 field 'pos'"), ([(0.5, 1.0, 0.0)] + GOOD_POINTS[1:], "point 0 field 'pos'"),
                         (GOOD_POINTS[:2] + [(0.0, 4.5, 0.0)], "point 2 field 'ratio'"), (GOOD_POINTS[:2] + [(0.0, 0.2, 0.0)], "point 2 field 'ratio'"),
                         (GOOD_POINTS[:2] + [(0.0, float("nan"), 0.0)], "point 2 field 'ratio'"), (GOOD_POINTS[:2] + [(0.0, 1.0, float("inf"))], "point 2 field 'cum'"),
                         (GOOD_POINTS[:2] + [(0.0, 1.0)], "point 2 has 2 fields")):
        with pytest.raises(ValueError, match="note_warp: " + message):
            kernels.note_warp_table(GOOD_NOTES, bad, GOOD_FIRST, 4, 1024)
    for bad, message in (([0, 2, 2, 3], "curve 1 has no point"), ([1, 2, 3], "first must run from 0"), ([0, 2, 4], "first must run from 0"), ([0, 2.0, 3], "first\\[1\\]")):
        with pytest.raises(ValueError, match="note_warp: " + message):
            kernels.note_warp_table(GOOD_NOTES, GOOD_POINTS, bad, 4, 1024)
    with pytest.raises(ValueError, match="note_warp: the table is empty"):
        kernels.note_warp_table([], GOOD_POINTS, GOOD_FIRST, 4, 1024)


REFUSALS = [("n_notes", 0, b"n_notes"), ("n_notes", 65536, b"n_notes"), ("rows", 0, b"rows"), ("length", 0, b"length"), ("length", (1 << 30) + 1, b"length"),
            ("row_stride", 1023, b"row_stride"), ("n_curves", 0, b"n_curves"), ("n_points", 0, b"n_points"), ("n_points", -1, b"n_points"),
            ("waves", None, b"null"), ("notes", None, b"null"), ("points", None, b"null"), ("first", None, b"null"), ("table", None, b"null"),
            ("waves", 0x10002, b"misaligned"), ("notes", 0x10004, b"misaligned"), ("points", 0x10004, b"misaligned"), ("first", 0x10002, b"misaligned"),
            ("table", 0x10008, b"misaligned")]


def warp_args(**change):
    P = 0x10000   # (never dereferenced: the argument checks come first and nothing is launched)
    good = dict(waves=P, rows=4, length=1024, row_stride=1024, notes=P, n_notes=2, points=P, first=P, n_curves=2, n_points=3, table=P, stream=None)
    return list(dict(good, **change).values())


def test_note_warp_refusals_without_gpu():
    from gansynth_amd import _lib
    lib = _lib.load()
    for field, value, message in REFUSALS:
        assert lib.gs_note_warp(*warp_args(**{field: value})) == -1, (field, value)       # GS_ERR_ARG
        assert message in lib.gs_last_error() and b"note_warp" in lib.gs_last_error(), (field, value, lib.gs_last_error())


# -------------------------------------------------------------------------------------------------------- driver and model
def test_bend_flag():
    import gan_synth_main as main
    args = main.parser.parse_args(["--synthesize", "score.mid"])
    assert args.bend is False and main.check_controller_args(args) is False
    args = main.parser.parse_args(["--synthesize", "a.mid", "--bend", "--controller_ramp", "0.05"])       # the ramp is shared
    assert args.bend is True and args.controller_ramp == 0.05 and main.check_controller_args(args) is False
    for argv, message in ((["--bend"], "--bend applies to --synthesize only"), (["--synthesize", "a.mid", "--bend", "--controller_ramp", "-1"], "non-negative"),
                          (["--synthesize", "a.mid", "--controller_ramp", "0.02"], "needs --controllers")):
        with pytest.raises(SystemExit, match=message):
            main.check_controller_args(main.parser.parse_args(argv))


def test_synthesize_takes_bend():
    from gansynth_amd.models import GANSynth
    assert inspect.signature(GANSynth.synthesize).parameters["bend"].default is False
