"""GPU: gs_loop_search against tests/sustain_ref.py within four times the error of its fp32 restatement, gs_note_sustain against the fp32
restatement bit for bit, untouched sentinels around every destination and around the scores, bad tables that the kernels must skip,
the Python layer's refusals, and GANSynth.synthesize(sustain=True) end to end on the reduced PGGAN of tests/test_notes_gpu.py."""
import numpy as np
import pytest
import torch

from tests import controllers_ref as CRF
from tests import stereo_ref as STR
from tests import sustain_ref as S
from tests import synth_ref as SR
from tests.test_notes_cpu import END, header, track
from tests.test_sustain_cpu import BAD_JOBS, BAD_SEARCH, GOOD_JOBS, GOOD_SEARCH

pytestmark = pytest.mark.gpu
PAD = 64
MARGIN = 4      # the project's margin between a kernel and the fp32 restatement of its rule (tests/test_loudness_gpu.py)
GAP = 3         # sentinels between two notes' rows of scores
NAN = float("nan")


def _K():
    from gansynth_amd import kernels
    return kernels.get()


def _upload(arr):
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _buffer(sources, rows, length, stride):
    """[rows, length] with rows `stride` apart inside a buffer of sentinels: `sources` (row -> samples) sit between rows of NaN with NaN
    in their stride padding; every other row, and the pads around the whole, hold the sentinel."""
    buf = torch.full((PAD + rows * stride + PAD,), S.SENTINEL, dtype=torch.float32)
    view = buf[PAD:PAD + rows * stride].view(rows, stride)
    for r, x in sources.items():
        view[r - 1] = view[r + 1] = NAN
    for r, x in sources.items():
        view[r] = NAN
        view[r, :length] = torch.from_numpy(x)
    return buf


# ------------------------------------------------------------------------------------------------------------- the search
SEARCH_ROWS = 8                            # NaN, the six rows of sustain_ref.search_rows, NaN
SEARCH_CASES = {                           # name -> (length, stride, a, m_min, m_max, W)
    "the tones' plan": (S.LENGTH, S.STRIDE) + S.TONE_PLAN,
    "W 16": (S.LENGTH, S.STRIDE, 900, 400, 900, 16),
    "W 255": (S.LENGTH, S.STRIDE, 900, 400, 900, 255),
    "W 257": (S.LENGTH, S.STRIDE, 900, 400, 900, 257),
    "W 4096": (6000, 6004, 100, 400, 700, 4096),
    "1 lag": (S.LENGTH, S.STRIDE, 900, 858, 858, 256),
    "255 lags": (S.LENGTH, S.STRIDE, 900, 400, 654, 256),
    "256 lags": (S.LENGTH, S.STRIDE, 900, 400, 655, 256),
    "257 lags": (S.LENGTH, S.STRIDE, 900, 400, 656, 256),
}


def _search_raw(x, length, stride, notes, n_lags):
    """gs_loop_search itself on the table AS GIVEN (no validation), the waves inside _buffer and the scores inside sentinels, GAP of them
    between the notes' rows -> scores [len(notes), n_lags + GAP] on the host, after checking the call and the pads around the scores and
    that the waves are as they were."""
    from gansynth_amd import _lib, kernels
    K = _K()
    buf = _buffer({1 + r: row for r, row in enumerate(x)}, SEARCH_ROWS, length, stride)
    dev = buf.cuda()
    nts = _upload((_lib.GsLoopNote * len(notes))(*[_lib.GsLoopNote(*[int(v) for v in note], 0) for note in notes]))
    scores = torch.full((PAD + len(notes) * (n_lags + GAP) + PAD,), S.SENTINEL, dtype=torch.float32, device="cuda")
    code = K.lib.gs_loop_search(dev[PAD:].data_ptr(), SEARCH_ROWS, length, stride, nts.data_ptr(), len(notes), scores[PAD:].data_ptr(),
                                n_lags + GAP, kernels._stream())
    torch.cuda.synchronize()
    assert code == 0, K.lib.gs_last_error()
    assert np.array_equal(dev.cpu().numpy(), buf.numpy(), equal_nan=True)
    got = scores.cpu().numpy()
    assert (got[:PAD] == S.SENTINEL).all() and (got[-PAD:] == S.SENTINEL).all()
    return got[PAD:-PAD].reshape(len(notes), n_lags + GAP)


@pytest.fixture(scope="module")
def search_reference():
    """name -> (rows, float64 scores [6, lags], fp32 restatement [6, lags]), once."""
    out = {}
    for name, (length, _, a, m_min, m_max, W) in SEARCH_CASES.items():
        x = S.search_rows(length)
        out[name] = (x, np.stack([S.scores_f64(r, a, m_min, m_max, W) for r in x]), np.stack([S.scores_f32(r, a, m_min, m_max, W) for r in x]))
    return out


@pytest.mark.parametrize("name", list(SEARCH_CASES))
def test_loop_search_against_the_restatement(search_reference, name):
    from gansynth_amd import notes as N
    length, stride, a, m_min, m_max, W = SEARCH_CASES[name]
    x, s64, s32 = search_reference[name]
    n_lags = m_max - m_min + 1
    notes = [(1 + r, a, m_min, m_max, W) for r in range(len(x))]
    got = _search_raw(x, length, stride, notes, n_lags)
    assert (got[:, n_lags:] == S.SENTINEL).all()
    got = got[:, :n_lags]
    e_kernel, e_f32 = np.abs(got - s64).max(), np.abs(s32 - s64).max()
    print(f"{name}: e(kernel) = {e_kernel:.3g}, e(scores_f32) = {e_f32:.3g}, ratio {e_kernel / e_f32 if e_f32 else 0:.2f}")
    assert np.isfinite(got).all() and e_kernel <= MARGIN * e_f32, (name, e_kernel, e_f32)
    assert (got[4] == 0).all()                                                               # the silent row
    for r in range(len(x)):                                                                  # the host pick from the kernel's scores
        m = N.pick_loop(got[r], m_min)
        assert s64[r, m - m_min] >= s64[r].max() - (1e-3 + 2 * e_kernel), (name, r, m)
        if name == "the tones' plan" and r < 4:
            assert abs(m - round(m / S.PERIODS[r]) * S.PERIODS[r]) <= 1, (r, m)
    again = _search_raw(x, length, stride, notes, n_lags)[:, :n_lags]                        # two calls are bit-identical
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def test_loop_search_skips_bad_notes(search_reference):
    """Bad tables handed to the entry point itself: every bad note is judged before an address is formed from it, its scores stay
    sentinels, and the good notes' scores are bit for bit those of a call without the bad ones."""
    length, stride, a, m_min, m_max, W = SEARCH_CASES["257 lags"]
    x = search_reference["257 lags"][0]
    n_lags = m_max - m_min + 1
    good = [(1, a, m_min, m_max, W), (6, a, m_min + 7, m_max, W - 3)]
    want = _search_raw(x, length, stride, good, n_lags)
    big = 2 ** 31 - 1
    bad = [(-1, a, m_min, m_max, W), (SEARCH_ROWS, a, m_min, m_max, W), (big, a, m_min, m_max, W), (1, -1, m_min, m_max, W), (1, a, 0, 200, W),
           (1, a, -5, 200, W), (1, a, m_min, m_min - 1, W), (1, a, m_min, m_max, 0), (1, a, m_min, m_max, -1), (1, a, m_min, m_max, 4097),
           (1, a, m_min, length - a - W + 1, W), (1, big, big - 10, big, 4096), (1, a, m_min - GAP - 1, m_max, W), (1, a, 1, big, 1)]
    got = _search_raw(x, length, stride, bad[:5] + good[:1] + bad[5:9] + good[1:] + bad[9:], n_lags)
    keep = [5, 10]
    assert np.array_equal(got[keep].view(np.uint32), want.view(np.uint32))
    assert (np.delete(got, keep, axis=0) == S.SENTINEL).all()


# ----------------------------------------------------------------------------------------------------------- the waveform
SRC_A, SRC_B = 1, 3
DSTS = (5, 7, 9, 11, 13)                    # sentinel rows between them and behind them
SUSTAIN_ROWS = 15
TONE_A, TONE_M = 900, 864                   # the loop of the 61.7-sample tone (tests/test_sustain_cpu.py has the pick)


@pytest.fixture(scope="module")
def sources():
    return {SRC_A: S.tone(61.7), SRC_B: S.tone(37.3, seed=6)}


def _sustain_raw(sources, jobs):
    """gs_note_sustain itself on the table AS GIVEN -> the rows [SUSTAIN_ROWS, STRIDE] on the host, after checking the call and the pads."""
    from gansynth_amd import _lib, kernels
    K = _K()
    buf = _buffer(sources, SUSTAIN_ROWS, S.LENGTH, S.STRIDE).cuda()
    table = _upload((_lib.GsSustainJob * len(jobs))(*[_lib.GsSustainJob(*[int(v) for v in job]) for job in jobs]))
    code = K.lib.gs_note_sustain(buf[PAD:].data_ptr(), SUSTAIN_ROWS, S.LENGTH, S.STRIDE, table.data_ptr(), len(jobs), kernels._stream())
    torch.cuda.synchronize()
    assert code == 0, K.lib.gs_last_error()
    got = buf.cpu().numpy()
    assert (got[:PAD] == S.SENTINEL).all() and (got[-PAD:] == S.SENTINEL).all()
    return got[PAD:-PAD].reshape(SUSTAIN_ROWS, S.STRIDE)


def _check_jobs(sources, rows, jobs):
    """Every job's destination holds the fp32 restatement bit for bit in [0, count); everything else is as _buffer left it."""
    want = _buffer(sources, SUSTAIN_ROWS, S.LENGTH, S.STRIDE).numpy()[PAD:-PAD].reshape(SUSTAIN_ROWS, S.STRIDE).copy()
    for src, dst, offset, count, a, m, xfade in jobs:
        want[dst, :count] = S.sustained_f32(sources[src], a, m, xfade, offset, count)
    assert np.array_equal(rows.view(np.uint32), want.view(np.uint32))


B_, X_ = TONE_A + TONE_M, S.TONE_XFADE


@pytest.mark.parametrize("offset", [0, B_ - 1, B_, B_ + X_ - 1, B_ + X_, 3_000_000_007])
def test_note_sustain_bit_for_bit(sources, offset):
    """Counts around the tile of 1024, one per destination, alternating between the two sources (two jobs read one source)."""
    jobs = [(SRC_A if j % 2 == 0 else SRC_B, dst, offset, count, TONE_A, TONE_M, X_) for j, (dst, count) in
            enumerate(zip(DSTS, (1, 1023, 1024, 1025, S.LENGTH)))]
    _check_jobs(sources, _sustain_raw(sources, jobs), jobs)


def test_note_sustain_edges_of_the_rule(sources):
    """No crossfade, a crossfade of one sample, a loop of one sample, and loops that end at the row's end exactly."""
    jobs = [(SRC_A, 5, 0, S.LENGTH, TONE_A, TONE_M, 0), (SRC_A, 7, 1700, S.LENGTH, TONE_A, TONE_M, 1), (SRC_B, 9, 0, S.LENGTH, 900, 1, 1),
            (SRC_B, 11, 5, S.LENGTH, 2000, 901, 100), (SRC_A, 13, 2999, 2000, 0, S.LENGTH, 0)]
    assert 2000 + 901 + 100 == S.LENGTH
    rows = _sustain_raw(sources, jobs)
    _check_jobs(sources, rows, jobs)
    assert np.array_equal(rows[5, :TONE_A + TONE_M], sources[SRC_A][:TONE_A + TONE_M])      # up to b the note itself
    assert np.array_equal(rows[13, 2:2000], sources[SRC_A][:1998])                           # the whole row as the loop: it starts over
    again = _sustain_raw(sources, jobs)
    assert np.array_equal(rows.view(np.uint32), again.view(np.uint32))


def test_note_sustain_at_the_headline_size():
    """200 notes of 64000 samples held 8 s under a release of 1 s -- three pieces a note, 150 000 waves -- bit for bit.  At this size
    an earlier form of the kernel, which kept the loop position in 64 bits, got the crossfade weight of one wave in some ten thousand
    wrong by a power of two (DESIGN.md "Sustain"); the small cases above never showed it."""
    from gansynth_amd import notes as N
    K = _K()
    notes, length = 200, 64000
    a, m_min, m_max, _, xfade = N.sustain_plan(length)
    pieces = N.sustain_pieces(8 * 16000, 16000, length)
    assert [h + r for _, h, r in pieces] == [64000, 16000, 64000]
    rng = np.random.default_rng(3)
    x = (rng.random((notes, length), dtype=np.float32) - np.float32(0.5))
    loops = rng.integers(m_min, m_max + 1, notes)
    waves = torch.full((notes * 4, length), S.SENTINEL, device="cuda")
    waves[:notes] = torch.from_numpy(x).cuda()
    jobs = [(n, notes + 3 * n + j, off, h + r, a, int(loops[n]), xfade) for n in range(notes) for j, (off, h, r) in enumerate(pieces)]
    K.note_sustain(waves, jobs)
    got = waves[notes:].cpu().numpy().reshape(notes, 3, length)
    for n in range(notes):
        y = S.sustained_f32(x[n], a, int(loops[n]), xfade, 0, pieces[-1][0] + length)
        for j, (off, h, r) in enumerate(pieces):
            assert np.array_equal(got[n, j, :h + r], y[off:off + h + r]) and (got[n, j, h + r:] == S.SENTINEL).all(), (n, j)


def test_note_sustain_skips_bad_jobs(sources):
    """Bad tables handed to the entry point itself: every bad job is judged before an address is formed from it; the result is that of
    the good jobs alone, bit for bit, and nothing else is written."""
    good = [(SRC_A, 5, 1000, 2500, TONE_A, TONE_M, X_), (SRC_B, 9, 0, S.LENGTH, 900, 300, 7)]
    big, L = 2 ** 31 - 1, S.LENGTH
    bad = [(-1, 7, 0, 100, 900, 300, 7), (SUSTAIN_ROWS, 7, 0, 100, 900, 300, 7), (big, 7, 0, 100, 900, 300, 7), (SRC_A, -1, 0, 100, 900, 300, 7),
           (SRC_A, SUSTAIN_ROWS, 0, 100, 900, 300, 7), (SRC_A, big, 0, 100, 900, 300, 7), (7, 7, 0, 100, 900, 300, 7), (SRC_A, 7, 0, 0, 900, 300, 7),
           (SRC_A, 7, 0, -5, 900, 300, 7), (SRC_A, 7, 0, L + 1, 900, 300, 7), (SRC_A, 7, 0, big, 900, 300, 7), (SRC_A, 7, -1, 100, 900, 300, 7),
           (SRC_A, 7, -2 ** 63, 100, 900, 300, 7), (SRC_A, 7, 0, 100, -1, 300, 7), (SRC_A, 7, 0, 100, 900, 0, 7), (SRC_A, 7, 0, 100, 900, -3, 7),
           (SRC_A, 7, 0, 100, 900, 300, -1), (SRC_A, 7, 0, 100, 900, 300, L - 1199), (SRC_A, 7, 0, 100, big, big, big), (SRC_A, 7, 4000, 100, L, 1, 0)]
    rows = _sustain_raw(sources, bad[:10] + good[:1] + bad[10:15] + good[1:] + bad[15:])
    _check_jobs(sources, rows, good)
    assert (rows[7] == S.SENTINEL).all()


def test_the_python_layer(sources):
    K = _K()
    waves = torch.zeros(4, 1024, device="cuda")
    for bad, message in BAD_SEARCH:
        if len(bad) == 5 and bad[2] != 49:   # (one plan serves every note of loop_search, and it sizes the scores itself)
            with pytest.raises(ValueError, match="loop_search: " + message):
                K.loop_search(waves, [bad[0], 1], bad[1:])
    for bad, message in BAD_JOBS:
        with pytest.raises(ValueError, match="note_sustain: " + message):
            K.note_sustain(waves, [bad, GOOD_JOBS[1]])
    for call in (lambda w: K.loop_search(w, [0], GOOD_SEARCH[0][1:]), lambda w: K.note_sustain(w, GOOD_JOBS)):
        with pytest.raises(ValueError, match="waves must be"):
            call(waves.double())
        with pytest.raises(ValueError, match="the rows of waves"):
            call(waves.t())
    assert (waves == 0).all()
    # through the Python layer: the scores of the plan, the rows written in place
    a, m_min, m_max, W = S.TONE_PLAN
    waves = torch.zeros(SUSTAIN_ROWS, S.LENGTH, device="cuda")
    for r, x in sources.items():
        waves[r] = torch.from_numpy(x).cuda()
    scores = K.loop_search(waves, [SRC_A, SRC_B], S.TONE_PLAN + (S.TONE_XFADE,))          # (a plan of five, as sustain_plan gives it)
    assert scores.shape == (2, m_max - m_min + 1) and scores.dtype == torch.float32
    for i, r in enumerate((SRC_A, SRC_B)):
        s64 = S.scores_f64(sources[r], a, m_min, m_max, W)
        assert np.abs(scores[i].cpu().numpy() - s64).max() <= MARGIN * np.abs(S.scores_f32(sources[r], a, m_min, m_max, W) - s64).max()
    jobs = [(SRC_A, 5, 700, 2000, TONE_A, TONE_M, X_), (SRC_A, 7, 2700, S.LENGTH, TONE_A, TONE_M, X_)]
    assert K.note_sustain(waves, jobs) is waves
    for src, dst, offset, count, a, m, xfade in jobs:
        assert np.array_equal(waves[dst, :count].cpu().numpy(), S.sustained_f32(sources[src], a, m, xfade, offset, count)) and (waves[dst, count:] == 0).all()
    # the two pieces butt: the second starts where the first stopped
    assert np.array_equal(S.sustained_f32(sources[SRC_A], TONE_A, TONE_M, X_, 700, 2301)[2000:], waves[7, :301].cpu().numpy())


# ---------------------------------------------------------------------------------------------------------- end to end
KW = dict(batch_size=4, release_seconds=0.01, seconds_per_instrument=0.04, seed=2)
SR_HZ, L = 16000, 1024


def at(tick):   # the tempo map's own arithmetic: 500000 microseconds a quarter of 480 ticks, 960 ticks a second
    return tick * 500000 / (480 * 1e6)


def _held_score():
    """Format 1, 960 ticks a second, two channels.  A lasts 8 s.  B and C end under a pedal that goes up at tick 230: with controllers
    they last 200 and 130 ticks, past the 61 of the waveform; without, 20 and 30.  D, on channel 2, is short."""
    one = track([
        (0, [0x90, 60, 100]),        # tick 0     A on
        (30, [0x90, 67, 90]),        # tick 30    B on
        (5, [0xB0, 64, 127]),        # tick 35    pedal down
        (15, [0x80, 67, 0]),         # tick 50    B off under the pedal
        (50, [0x90, 72, 127]),       # tick 100   C on
        (30, [0x80, 72, 0]),         # tick 130   C off under the pedal
        (100, [0xB0, 64, 0]),        # tick 230   pedal up
        (7450, [0x80, 60, 0]),       # tick 7680  A off: 8 s
        (0, END)])
    two = track([(0, [0xC1, 33]), (0, [0xB1, 10, 100]), (10, [0x91, 48, 80]), (40, [0x81, 48, 0]), (0, END)])
    return header(1, 2, 480) + one + two


def _short_score():
    return header(1, 1, 480) + track([(0, [0x90, 60, 100]), (30, [0x80, 60, 0]), (10, [0x90, 64, 50]), (40, [0x80, 64, 0]), (0, END)])


def test_sustain_on_a_score_that_fits_changes_nothing(gpu_store):
    from tests.test_notes_gpu import _model
    K = _K()
    model = _model()
    for how in (dict(), dict(ensemble=True, stereo=True, spread=0.5), dict(controllers=True, stereo=True)):
        launches = (K.loop_searches, K.note_sustains)
        want, want_pcm = model.synthesize(_short_score(), want_pcm=True, **how, **KW)
        info = {}
        got, pcm = model.synthesize(_short_score(), want_pcm=True, sustain=True, info=info, **how, **KW)
        assert torch.equal(got, want) and torch.equal(pcm, want_pcm) and (K.loop_searches, K.note_sustains) == launches
        assert (info["held_notes"], info["sustain_rows"], info["loops"], info["sustain_cut_bent"]) == (0, 0, [], 0)


def _reference_rows(model, info, held):
    """The waves buffer as sustain_ref builds it from the generated rows: -> (rows fp32 [N + pieces, L], table, total, owner, offset)."""
    from gansynth_amd import notes as N
    from tests.test_ensemble_gpu import _hand_waves
    K = _K()
    waves = _hand_waves(model, info, 4)
    a, m_min, m_max, W, X = S.sustain_plan(L)
    notes = [tuple(n) for n in info["notes"]]
    table, total, kept, _, owner, offset = S.schedule_sustain(notes, range(24, 85), SR_HZ, L, 0.01)
    assert kept == list(range(len(notes))) and sorted({n for n, off in zip(owner, offset) if off is not None}) == held
    assert info["held_notes"] == len(held) and info["sustain_rows"] == sum(off is not None for off in offset) and info["total_samples"] == total
    # the loops: the host pick from the kernel's scores of the generated rows, held to the float64 scores
    scores = K.loop_search(waves, held, (a, m_min, m_max, W)).cpu().numpy()
    host = waves.cpu().numpy()
    loops = {}
    for i, n in enumerate(held):
        s64 = S.scores_f64(host[n], a, m_min, m_max, W)
        e = np.abs(scores[i] - s64).max()
        m = N.pick_loop(scores[i], m_min)
        assert e <= MARGIN * np.abs(S.scores_f32(host[n], a, m_min, m_max, W) - s64).max() and s64[m - m_min] >= s64.max() - (1e-3 + 2 * e)
        assert info["loops"][i] == (a, m, float(scores[i, m - m_min]))
        loops[n] = m
    return S.piece_rows(host, table, owner, offset, loops, a, X, "f32"), table, total, owner, offset


def test_a_held_score_is_the_mix_over_the_looped_rows(gpu_store):
    """The plain path.  The clip is as long as the score says, it is synth_ref's float64 mix over sustain_ref's rows -- the fp32 rows
    that gs_note_sustain is held to bit for bit above -- within synth_ref's bound, and it sounds past the generated length."""
    from tests.test_notes_gpu import _model
    K = _K()
    model = _model()
    info, plain_info = {}, {}
    launches = (K.loop_searches, K.note_sustains)
    clip = model.synthesize(_held_score(), sustain=True, normalize=False, info=info, **KW)
    assert (K.loop_searches, K.note_sustains) == (launches[0] + 1, launches[1] + 1)
    plain = model.synthesize(_held_score(), normalize=False, info=plain_info, **KW)
    assert [n.pitch for n in info["notes"]] == [60, 48, 67, 72] and info["notes"][0].end == at(7680)
    assert clip.shape == (8 * SR_HZ + 160,) and info["total_samples"] == 8 * SR_HZ + 160 and plain_info["total_samples"] == at_sample(100) + 500 + 160
    rows, table, total, owner, offset = _reference_rows(model, info, [0])                    # A alone: without controllers the pedal is not read
    assert len(table) == 3 + 126 and table[0][:4] == (0, L, 0, 4) and table[125][:4] == (124 * L + 160, L - 160, 160, 4 + 125)
    ref, a, m = SR.mix(rows, table, total)
    got = clip.cpu().numpy()
    assert (np.abs(got.astype(np.float64) - ref) <= SR.bound(a, m)).all()
    assert np.array_equal(got, SR.mix_f32(rows, table, total))
    assert np.abs(got[4 * L:8 * SR_HZ]).max() > 0 and np.abs(got[4 * SR_HZ:8 * SR_HZ]).max() > 0        # past the waveform, past four seconds
    b = info["loops"][0][0] + info["loops"][0][1]
    assert np.array_equal(got[:min(b, at_sample(10))], plain.cpu().numpy()[:min(b, at_sample(10))])   # until another note or the loop: as before


def at_sample(tick):
    return int(np.floor(at(tick) * SR_HZ + 0.5))


def test_a_held_score_in_stereo_and_under_controllers(gpu_store):
    from gansynth_amd import notes as N
    from tests.test_notes_gpu import _model
    model = _model()
    data = _held_score()
    # stereo, parts: the pieces carry their note's two gains
    info = {}
    clip, pcm = model.synthesize(data, sustain=True, ensemble=True, stereo=True, spread=0.5, normalize=False, want_pcm=True, info=info, **KW)
    rows, table, total, owner, offset = _reference_rows(model, info, [0])
    score = N.read_score(data)
    gains = N.schedule_gains(N.kept_indices(score.notes, range(24, 85)), score, 0.5)
    stereo_table = [row[:4] + gains[n] for row, n in zip(table, owner)]
    ref, a, m = STR.mix(rows, stereo_table, total)
    got = clip.cpu().numpy()
    assert clip.shape == (2, 8 * SR_HZ + 160) and pcm.shape == (8 * SR_HZ + 160, 2)
    assert (np.abs(got.astype(np.float64) - ref) <= SR.bound(a, m[None])).all() and np.array_equal(got, STR.mix_f32(rows, stereo_table, total))
    assert np.abs(got[:, 4 * L:8 * SR_HZ]).max() > 0 and np.array_equal(pcm.cpu().numpy(), SR.pcm16(got).T)
    # controllers: the pedal holds B and C past the waveform as well, and the pieces carry their part's curve
    info = {}
    clip = model.synthesize(data, sustain=True, controllers=True, controller_ramp=0.001, normalize=False, info=info, **KW)
    assert info["pedal_extended"] == 2 and [(n.pitch, n.end) for n in info["notes"]][2:] == [(67, at(230)), (72, at(230))]
    rows, table, total, owner, offset = _reference_rows(model, info, [0, 2, 3])
    performance = N.read_performance(data)
    index = N.kept_indices(performance.score.notes, range(24, 85))
    points, first = N.schedule_curves(performance, index, SR_HZ, 0.001, False, 0.0)
    curve_table = [row + (performance.score.part[index[n]],) for row, n in zip(table, owner)]
    ref, a, m = CRF.mix(rows, curve_table, points, first, total, 1)
    got = clip.cpu().numpy()
    assert clip.shape == (8 * SR_HZ + 160,)
    assert (np.abs(got.astype(np.float64) - ref[0]) <= CRF.bound(a, m[None])[0]).all()
    assert np.array_equal(got, CRF.mix_f32(rows, curve_table, points, first, total, 1)[0])
    assert np.abs(got[4 * L:8 * SR_HZ]).max() > 0


def test_a_held_note_that_bends_is_cut_as_before(gpu_store):
    from tests.test_notes_gpu import _model
    K = _K()
    model = _model()
    bends = [[(at(20), 1.0)], []]                                                            # part 0 bends while A sounds
    want_info, info = {}, {}
    want = model.synthesize(_held_score(), bend=bends, controller_ramp=0.001, info=want_info, **KW)
    launches = (K.loop_searches, K.note_sustains)
    got = model.synthesize(_held_score(), bend=bends, controller_ramp=0.001, sustain=True, info=info, **KW)
    assert torch.equal(got, want) and (K.loop_searches, K.note_sustains) == launches
    assert (info["sustain_cut_bent"], info["held_notes"], info["sustain_rows"]) == (1, 0, 0) and info["total_samples"] == want_info["total_samples"]
    # a bend on the other part leaves A held
    info = {}
    clip = model.synthesize(_held_score(), bend=[[], [(at(20), 1.0)]], controller_ramp=0.001, sustain=True, info=info, **KW)
    assert (info["sustain_cut_bent"], info["held_notes"], info["bent_notes"]) == (0, 1, 1) and clip.shape == (8 * SR_HZ + 160,)


def test_a_train_step_after_a_sustained_synthesize_is_the_same_step():
    from gansynth_amd import variables
    from oracle import torch_ref as R
    from tests.test_model_gpu import cuda
    from tests.test_notes_gpu import _model
    old = variables._default
    losses = []
    try:
        for with_synthesize in (False, True):
            variables.set_default_store(variables.VariableStore(device="cuda"))
            torch.manual_seed(17)
            model = _model()
            if with_synthesize:
                info = {}
                model.synthesize(_held_score(), sustain=True, info=info, **KW)
                assert info["held_notes"] == 1
            lat, lab, real = R.synthetic_batch(4, rank=1, image_shape=(2, 16, 128))
            d = torch.as_tensor(model.discriminator_step(cuda(lat), cuda(lab), cuda(real))).detach().clone()
            g = torch.as_tensor(model.generator_step(cuda(lat), cuda(lab))).detach().clone()
            losses.append((d, g, model.g_params.flat.clone(), model.d_params.flat.clone()))
    finally:
        variables._default = old
    for a, b in zip(*losses):
        assert torch.equal(a, b)


def test_driver_with_sustain(gpu_store, tmp_path):
    """What `gan_synth_main.py --synthesize organ.mid --sustain` runs after building its model."""
    from scipy.io import wavfile
    import gan_synth_main as main
    from tests.test_notes_gpu import _model
    model = _model()
    (tmp_path / "organ.mid").write_bytes(_held_score())
    argv = ["--synthesize", str(tmp_path / "organ.mid"), "--batch_size", "4", "--release_seconds", "0.01", "--model_dir", str(tmp_path / "no_model")]
    lines = []
    info = main.synthesize_to_wav(model, main.parser.parse_args(argv + ["--output", str(tmp_path / "held.wav"), "--sustain"]), range(24, 85),
                                  log=lines.append)
    m = info["loops"][0][1]
    assert lines[-1] == f"sustain: 1 notes held in 126 pieces, loops of {m} to {m} samples, 0 held notes cut because they bend"
    plain_lines = []
    plain_info = main.synthesize_to_wav(model, main.parser.parse_args(argv + ["--output", str(tmp_path / "plain.wav")]), range(24, 85), log=plain_lines.append)
    assert "held_notes" not in plain_info and not any(line.startswith("sustain:") for line in plain_lines)
    rate, held = wavfile.read(str(tmp_path / "held.wav"))
    _, plain = wavfile.read(str(tmp_path / "plain.wav"))
    assert rate == SR_HZ and held.shape == (8 * SR_HZ + 160,) and plain.shape == (plain_info["total_samples"],) and np.abs(held[4 * L:]).max() > 0
