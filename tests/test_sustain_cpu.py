"""No GPU: the sustain rules (DESIGN.md "Sustain") -- notes.sustain_plan, notes.pick_loop and notes.schedule_sustain against
tests/sustain_ref.py, the float64 rule on decaying test tones, the pieces against one long note in float64, the table builders'
refusals, the entry points' argument checks and the driver's flag."""
import inspect
import itertools

import numpy as np
import pytest

from tests import sustain_ref as S
from tests import synth_ref as SR


# --------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("length", [64, 3001, 64000])
def test_sustain_plan_bounds(length):
    from gansynth_amd import notes as N
    a, m_min, m_max, W, X = N.sustain_plan(length)
    assert (a, m_min, m_max, W, X) == S.sustain_plan(length)
    assert 0 <= a and 1 <= m_min <= m_max and W >= 16 and X >= 1 and a + m_max + max(W, X) <= length
    if length == 64000:
        assert (a, m_min, m_max, W, X) == (24000, 8000, 16000, 2000, 1000)


def test_sustain_plan_holds_for_every_length_and_refuses_short_ones():
    from gansynth_amd import notes as N
    for length in range(64, 5000):
        a, m_min, m_max, W, X = N.sustain_plan(length)
        assert 1 <= m_min <= m_max and a + m_max + max(W, X) <= length, length
    for length in (63, 1, 0):
        with pytest.raises(ValueError, match="sustain_plan"):
            N.sustain_plan(length)


# ------------------------------------------------------------------------------------------------------------- the pieces
def test_schedule_sustain_pieces_exhaustively():
    from gansynth_amd import notes as N
    L, sr = 10, 10
    for R, hold in itertools.product(range(10), range(1, 46)):
        score = [N.Note(60, 100, 0.3, 0.3 + hold / sr), N.Note(62, 50, 0.0, 0.1), N.Note(99, 50, 0.0, 0.2)]   # (1 + R <= L: never held)
        rows = [tuple(n) for n in score]
        kept, table, total, dropped, owner, offset = N.schedule_sustain(score, range(24, 85), sr, L, R / sr)
        want = S.schedule_sustain(rows, range(24, 85), sr, L, R / sr)
        assert (table, total, dropped, owner, offset) == (want[0], want[1], want[3], want[4], want[5]), (R, hold)
        assert [tuple(n) for n in kept] == [rows[i] for i in want[2]] and dropped == 1
        plain = N.schedule(score, range(24, 85), sr, L, R / sr)
        assert table[0] == plain[1][0] and owner[0] == 0 and offset[0] is None                # the short note: schedule's row
        mine = [(row, off) for row, n, off in zip(table, owner, offset) if n == 1]
        if hold + R <= L:
            assert mine == [(plain[1][1], None)] and total == plain[2] and len(table) == 2     # not held: schedule's rows exactly
            continue
        assert all(off is not None for _, off in mine)
        at = 0
        for j, ((onset, h, r, row, gain), off) in enumerate(mine):                           # the pieces tile [0, hold)
            assert off == at and onset == 3 + at and 1 <= h and h + r <= L and row == 2 + j and gain == 100 / 127.0
            assert r == (R if j == len(mine) - 1 else 0)                                       # only the last piece has the release
            at += h
        assert at == hold and total == 3 + hold + R
    with pytest.raises(ValueError, match="schedule_sustain: the release"):                   # R = L
        N.schedule_sustain([N.Note(60, 100, 0.0, 0.5)], range(24, 85), sr, L, L / sr)


def test_schedule_sustain_cut_keeps_schedules_row():
    from gansynth_amd import notes as N
    score = [N.Note(60, 100, 0.0, 3.0), N.Note(64, 100, 0.1, 3.0)]
    plain = N.schedule(score, range(24, 85), 10, 10, 0.2)
    _, table, total, _, owner, offset = N.schedule_sustain(score, range(24, 85), 10, 10, 0.2, cut=[0])
    assert table[0] == plain[1][0] and offset[0] is None and owner == [0, 1, 1, 1, 1] and [row[3] for row in table] == [0, 2, 3, 4, 5]
    assert total == 1 + 29 + 2


# --------------------------------------------------------------------------------------------------- the rule on the tones
@pytest.fixture(scope="module")
def tones():
    """period -> (x, float64 scores, the pick)."""
    a, m_min, m_max, W = S.TONE_PLAN
    out = {}
    for period in S.PERIODS:
        x = S.tone(period)
        scores = S.scores_f64(x, a, m_min, m_max, W)
        out[period] = (x, scores, S.pick_loop(scores, m_min))
    return out


def test_the_picks_on_the_tones_are_whole_periods(tones):
    from gansynth_amd import notes as N
    a, m_min, m_max, W = S.TONE_PLAN
    picks = []
    for period, (x, scores, m) in tones.items():
        assert N.pick_loop(scores, m_min) == m
        print(f"period {period}: m* = {m}, {m / period:.3f} periods, score {scores[m - m_min]:.6f}, max {scores.max():.6f}")
        assert abs(m - round(m / period) * period) <= 1 and scores.max() > 0.9999
        picks.append(m)
    assert picks == [858, 900, 864, 857]


def test_the_looped_tones_have_no_step_and_no_overshoot(tones):
    a = S.TONE_PLAN[0]
    for period, (x, _, m) in tones.items():
        b = a + m
        y = S.sustained_f64(x, a, m, S.TONE_XFADE, 0, 4 * S.LENGTH)
        assert np.array_equal(y[:b], x[:b].astype(np.float64))
        step, own = np.abs(np.diff(y[b - 2:])).max(), np.abs(np.diff(x.astype(np.float64))).max()
        print(f"period {period}: largest step of y from b - 2 on = {step / own:.3f} of x's own")
        assert step <= 1.0 * own
        assert np.abs(y[b:]).max() <= np.abs(x).max()


def test_the_looped_waveform_is_periodic_bit_for_bit(tones):
    a = S.TONE_PLAN[0]
    for kind in (S.sustained_f64, S.sustained_f32):
        for period, (x, _, m) in tones.items():
            b = a + m
            y = kind(x, a, m, S.TONE_XFADE, 0, b + 5 * m)
            tail = y[b + S.TONE_XFADE:]
            assert np.array_equal(tail[m:], tail[:-m])
            # a window that starts far out, past 2^31, is the same waveform: (k - b) mod m in 64 bits
            far = 3_000_000_007
            p = (far - b) % m
            assert np.array_equal(kind(x, a, m, S.TONE_XFADE, far, 500), kind(x, a, m, S.TONE_XFADE, b + m + p, 500))


def test_fp32_restatements_sit_next_to_float64(tones):
    a, m_min, m_max, W = S.TONE_PLAN
    for period, (x, scores, m) in tones.items():
        e = np.abs(S.scores_f32(x, a, m_min, m_max, W) - scores).max()
        y32, y64 = (f(x, a, m, S.TONE_XFADE, 0, 2 * S.LENGTH) for f in (S.sustained_f32, S.sustained_f64))
        print(f"period {period}: e(scores_f32) = {e:.3g}, max |y32 - y64| = {np.abs(y32 - y64).max():.3g}")
        assert e < 1e-5 and np.abs(y32 - y64).max() <= 3 * 2.0 ** -24 * np.abs(x).max()


# --------------------------------------------------------------------------------------------------------------- the pick
def test_pick_loop():
    from gansynth_amd import notes as N
    for pick in (N.pick_loop, S.pick_loop):
        assert pick([0.2, 0.9995, 0.5, 0.9991, 0.9984, 0.1], 10) == 13                         # within the tie of the best: the largest
        assert pick([0.2, 0.9995, 0.5, 0.9991, 0.9984, 0.1], 10, tie=0.0) == 11
        assert pick([1.0, 1.0, 1.0], 5) == 7                                                   # ties go to the largest lag
        assert pick([0.5, float("nan"), float("inf"), -float("inf")], 3) == 3                  # non-finite: -inf
        assert pick([float("nan"), -0.5, float("nan")], 3) == 4
        assert pick([0.0, 0.0, 0.0, 0.0], 100) == 103                                          # a silent row: m_max
        assert pick([0.0, float("nan"), 0.0, float("inf")], 100) == 103
        assert pick(np.float32([0.1, 0.3]), 1) == 2
    with pytest.raises(ValueError, match="pick_loop"):
        N.pick_loop([], 3)


# ----------------------------------------------------------------------------------- the pieces against one long note
@pytest.mark.parametrize("hold,release", [(3001 - 160, 160), (3001, 160), (3002, 160), (2 * 3001 + 1, 160), (9000, 0), (25000, 3000), (2842, 160)])
def test_the_pieces_are_one_long_note(tones, hold, release):
    """synth_ref's float64 mix of the piece table over rows cut from y IS one note that runs hold + R samples of y: an envelope of 1
    times a sample, and every sample covered by one piece -- no rounding differs, so the two are identical."""
    from gansynth_amd import notes as N
    sr, L = 16000, S.LENGTH
    x, _, m = tones[61.7]
    a = S.TONE_PLAN[0]
    note = N.Note(60, 90, 0.01, 0.01 + hold / sr)
    _, table, total, _, owner, offset = N.schedule_sustain([note], range(24, 85), sr, L, release / sr)
    assert sum(row[1] for row in table) == hold and table[-1][2] == release and total == 160 + hold + release
    if hold + release <= L:                                                                  # fits: schedule's row, the note as generated
        assert table == N.schedule([note], range(24, 85), sr, L, release / sr)[1] and offset == [None]
        return
    assert None not in offset
    waves = x[None]
    rows = S.piece_rows(waves, table, owner, offset, {0: m}, a, S.TONE_XFADE)
    got, _, covered = SR.mix(rows, table, total)
    want = S.mix_long_f64(x, a, m, S.TONE_XFADE, 160, hold, release, 90 / 127.0, total)
    assert covered[160:].min() == covered.max() == 1 and np.array_equal(got, want)
    if hold > 2 * L:                                                                         # and it sounds past the generated length
        assert np.abs(got[160 + L:160 + hold]).max() > 0.1 * np.abs(x).max()


# ------------------------------------------------------------------------------------------------------- table builders
GOOD_SEARCH = [(0, 100, 50, 200, 64), (1, 100, 50, 200, 64)]
BAD_SEARCH = [((-1, 100, 50, 200, 64), "note 0 field 'row'"), ((4, 100, 50, 200, 64), "note 0 field 'row'"), ((0, -1, 50, 200, 64), "note 0 field 'a'"),
              ((0, 100, 0, 150, 64), "note 0 field 'm_min'"), ((0, 100, 50, 49, 64), "note 0 field 'm_max'"), ((0, 100, 50, 200, 0), "note 0 field 'window'"),
              ((0, 100, 50, 200, 4097), "note 0 field 'window'"), ((0, 100, 50, 200, 725), "note 0 field 'm_max'"), ((0, 100, 49, 200, 64), "note 0 field 'm_max'"),
              ((0, 100, 50, 200.0, 64), "note 0 field 'm_max'"), ((0, 100, 50, True, 64), "note 0 field 'm_max'"), ((0, 100, 50, 200), "note 0 has 4 fields")]
GOOD_JOBS = [(0, 2, 0, 1024, 300, 200, 16), (1, 3, 3_000_000_007, 100, 300, 200, 0)]
BAD_JOBS = [((-1, 2, 0, 1024, 300, 200, 16), "job 0 field 'src_row'"), ((4, 2, 0, 1024, 300, 200, 16), "job 0 field 'src_row'"),
            ((0, 4, 0, 1024, 300, 200, 16), "job 0 field 'dst_row'"), ((0, -1, 0, 1024, 300, 200, 16), "job 0 field 'dst_row'"),
            ((0, 0, 0, 1024, 300, 200, 16), "job 0 field 'dst_row'"), ((0, 1, 0, 1024, 300, 200, 16), "job 0 field 'dst_row'"),
            ((0, 3, 0, 1024, 300, 200, 16), "job 1 field 'dst_row'"), ((0, 2, -1, 1024, 300, 200, 16), "job 0 field 'offset'"),
            ((0, 2, 2 ** 62, 1024, 300, 200, 16), "job 0 field 'offset'"), ((0, 2, 0, 0, 300, 200, 16), "job 0 field 'count'"),
            ((0, 2, 0, 1025, 300, 200, 16), "job 0 field 'count'"), ((0, 2, 0, 1024, -1, 200, 16), "job 0 field 'a'"),
            ((0, 2, 0, 1024, 300, 0, 16), "job 0 field 'm'"), ((0, 2, 0, 1024, 300, 200, -1), "job 0 field 'xfade'"),
            ((0, 2, 0, 1024, 300, 200, 525), "job 0 field 'xfade'"), ((0, 2, 0.5, 1024, 300, 200, 16), "job 0 field 'offset'"),
            ((0, 2, 0, 1024, 300, 200), "job 0 has 6 fields")]


def test_table_builders_refuse_every_bad_field():
    from gansynth_amd import kernels
    notes = kernels.loop_search_table(GOOD_SEARCH, 4, 1024, 151)
    assert [(n.row, n.a, n.m_min, n.m_max, n.window) for n in notes] == GOOD_SEARCH
    kernels.loop_search_table([(0, 100, 50, 200, 724)], 4, 1024, 151)                         # a + m_max + W == length exactly
    for bad, message in BAD_SEARCH:
        with pytest.raises(ValueError, match="loop_search: " + message):
            kernels.loop_search_table([bad, GOOD_SEARCH[1]], 4, 1024, 151)
    jobs = kernels.note_sustain_table(GOOD_JOBS, 4, 1024)
    assert [(j.src_row, j.dst_row, j.offset, j.count, j.a, j.m, j.xfade) for j in jobs] == GOOD_JOBS
    kernels.note_sustain_table([(0, 2, 0, 1024, 300, 200, 524)], 4, 1024)                     # a + m + xfade == length exactly
    for bad, message in BAD_JOBS:
        with pytest.raises(ValueError, match="note_sustain: " + message):
            kernels.note_sustain_table([bad, GOOD_JOBS[1]], 4, 1024)
    for build, args in ((kernels.loop_search_table, (4, 1024, 151)), (kernels.note_sustain_table, (4, 1024))):
        with pytest.raises(ValueError, match="the table is empty"):
            build([], *args)


REFUSALS = [("n", 0, b"1 to 65535"), ("n", 65536, b"1 to 65535"), ("rows", 0, b"rows"), ("length", 0, b"length"), ("length", (1 << 30) + 1, b"length"),
            ("row_stride", 1023, b"row_stride"), ("waves", None, b"null"), ("table", None, b"null"), ("waves", 0x10002, b"misaligned"),
            ("table", 0x10002, b"misaligned")]
SEARCH_REFUSALS = [("scores", None, b"scores"), ("scores", 0x10002, b"scores"), ("scores_stride", 0, b"scores_stride"),
                   ("scores_stride", (1 << 24) + 1, b"scores_stride")]


def sustain_args(search, **change):
    P = 0x10000   # (never dereferenced: the argument checks come first and nothing is launched)
    good = dict(waves=P, rows=4, length=1024, row_stride=1024, table=P, n=2)
    if search:
        good.update(scores=P, scores_stride=151)
    good.update(stream=None)
    return list(dict(good, **change).values())


def test_entry_point_refusals_without_gpu():
    from gansynth_amd import _lib
    lib = _lib.load()
    for search, fn, name in ((True, lib.gs_loop_search, b"loop_search"), (False, lib.gs_note_sustain, b"note_sustain")):
        for field, value, message in REFUSALS + (SEARCH_REFUSALS if search else []):
            assert fn(*sustain_args(search, **{field: value})) == -1, (name, field, value)       # GS_ERR_ARG
            assert message in lib.gs_last_error() and name in lib.gs_last_error(), (field, value, lib.gs_last_error())
    assert lib.gs_note_sustain(*sustain_args(False, table=0x10004)) == -1 and b"misaligned" in lib.gs_last_error()   # jobs: 8 bytes


def test_structs_mirror_the_header():
    import ctypes
    from gansynth_amd import _lib
    assert ctypes.sizeof(_lib.GsLoopNote) == 24 and ctypes.sizeof(_lib.GsSustainJob) == 32 and _lib.GsSustainJob.offset.offset == 8
    assert (_lib.SUSTAIN_MAX_WINDOW, _lib.SUSTAIN_LAG_TILE, _lib.SUSTAIN_TILE) == (4096, 256, 1024)


# -------------------------------------------------------------------------------------------------------- driver and model
def test_sustain_flag():
    import gan_synth_main as main
    args = main.parser.parse_args(["--synthesize", "score.mid"])
    assert args.sustain is False and main.check_controller_args(args) is False
    args = main.parser.parse_args(["--synthesize", "organ.mid", "--sustain"])
    assert args.sustain is True and main.check_controller_args(args) is False
    for argv in (["--sustain"], ["--sustain", "--generate"]):
        with pytest.raises(SystemExit, match="--sustain applies to --synthesize only"):
            main.check_controller_args(main.parser.parse_args(argv))


def test_synthesize_takes_sustain():
    from gansynth_amd.models import GANSynth
    assert inspect.signature(GANSynth.synthesize).parameters["sustain"].default is False
