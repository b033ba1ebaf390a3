"""GPU: gs_note_mix_curves against the stated fp32 order of tests/controllers_ref.py bit for bit and against its float64 mix within its
bound (M + 12) * 2^-24 * A, for one and two channels; against gs_note_mix and gs_note_mix_stereo under constant curves of 1; the finish
stage; both store paths; notes whose curve is out of range, which must be skipped; the entry point's refusals; and
GANSynth.synthesize(controllers=True) end to end on the reduced PGGAN of tests/test_notes_gpu.py.
tests/test_controllers_cpu.py::test_fp32_evaluation_sits_inside_the_bound shows on the CPU that the case has what it is meant to have."""
import numpy as np
import pytest
import torch

from tests import controllers_ref as CRF
from tests import stereo_ref as STR
from tests import synth_ref as SRF
from tests.test_notes_cpu import END, header, tempo, track

pytestmark = pytest.mark.gpu
L, TOTAL = STR.LENGTH, STR.TOTAL
SENTINEL, PCM_SENTINEL, PAD = 12345.0, 77, 64


def _K():
    from gansynth_amd import kernels
    return kernels.get()


def _upload(arr):
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _raw(waves, table, points, first, total, channels, normalize=False, want_pcm=False, want_peak=True, offset=0):
    """gs_note_mix_curves itself on the tables AS GIVEN (no validation, no sorting), `out` and `pcm` inside buffers full of a sentinel:
    -> (out [channels, total], pcm [total, channels] or None, peak or None) after checking that the call succeeded and that nothing but
    the rows' [0, total) and the PCM was written.  `offset`: floats by which the base of out is moved off its 16-byte alignment."""
    from gansynth_amd import _lib, kernels
    K = _K()
    stride = (total + 3) // 4 * 4
    notes = _upload((_lib.GsMixNoteCurve * len(table))(*[_lib.GsMixNoteCurve(int(o), int(h), int(r), int(row), float(g), int(c), 0)
                                                        for o, h, r, row, g, c in table]))
    pts = _upload((_lib.GsCurvePoint * len(points))(*[_lib.GsCurvePoint(int(p), float(l), float(r)) for p, l, r in points]))
    firsts = torch.tensor(first, dtype=torch.int32, device="cuda")
    buf = torch.full((PAD + offset + channels * stride + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[PAD + offset:PAD + offset + channels * stride].view(channels, stride)
    pbuf = torch.full((PAD + channels * total + PAD,), PCM_SENTINEL, dtype=torch.int16, device="cuda") if want_pcm else None
    pcm = pbuf[PAD:PAD + channels * total].view(total, channels) if want_pcm else None
    peak = torch.full((1,), -1.0, dtype=torch.float32, device="cuda") if want_peak else None
    ws = torch.empty(max(K.lib.gs_note_mix_curves_workspace_bytes(total), 256), dtype=torch.uint8, device="cuda")
    code = K.lib.gs_note_mix_curves(waves.data_ptr(), waves.shape[0], waves.shape[1], waves.stride(0), notes.data_ptr(), len(table),
                                    pts.data_ptr(), len(points), firsts.data_ptr(), len(first) - 1, channels, total, 1 if normalize else 0,
                                    out.data_ptr(), stride, None if pcm is None else pcm.data_ptr(), None if peak is None else peak.data_ptr(),
                                    ws.data_ptr(), ws.numel(), kernels._stream())
    torch.cuda.synchronize()
    assert code == 0, K.lib.gs_last_error()
    assert (buf[:PAD + offset] == SENTINEL).all() and (buf[PAD + offset + channels * stride:] == SENTINEL).all() and (out[:, total:] == SENTINEL).all()
    if want_pcm:
        assert (pbuf[:PAD] == PCM_SENTINEL).all() and (pbuf[PAD + channels * total:] == PCM_SENTINEL).all()
    return out[:, :total], pcm, peak


@pytest.fixture(scope="module")
def dense():
    """tests/controllers_ref.py's dense case, its waves as rows 1100 apart, the references and the kernel's unnormalised mixes: once."""
    waves, table, points, first = CRF.dense_case()
    dev = torch.from_numpy(waves).cuda()[:, :L]
    assert dev.stride(0) == STR.STRIDE
    case = dict(host=waves[:, :L], waves=dev, table=table, points=points, first=first)
    for ch in (1, 2):
        mix, _, peak = _raw(dev, table, points, first, TOTAL, ch)
        case[ch] = dict(mix=mix.clone(), peak=peak.clone())
    return case


ONES, ONES_FIRST = [(0, 1.0, 1.0)] * 5, [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("channels", [1, 2])
def test_bit_for_bit_the_stated_order(dense, channels):
    want = CRF.mix_f32(dense["host"], dense["table"], dense["points"], dense["first"], TOTAL, channels)
    got = dense[channels]["mix"].cpu().numpy()
    assert got.shape == (channels, TOTAL) and np.array_equal(got, want)
    assert float(dense[channels]["peak"]) == float(np.abs(want).max())
    only_mix, _, none = _raw(dense["waves"], dense["table"], dense["points"], dense["first"], TOTAL, channels, want_peak=False)   # the first launch alone
    assert none is None and torch.equal(only_mix, dense[channels]["mix"])
    # the left channel of two is the one channel of one
    assert torch.equal(dense[2]["mix"][0], dense[1]["mix"][0])


@pytest.mark.parametrize("channels", [1, 2])
def test_mix_against_the_reference(dense, channels):
    ref, a, m = CRF.mix(dense["host"], dense["table"], dense["points"], dense["first"], TOTAL, channels)
    got = dense[channels]["mix"].cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref)
    bound = CRF.bound(a, m[None])
    bad = np.argwhere(~(err <= bound))                                     # (NaN fails)
    assert bad.size == 0, (len(bad), bad[:4].tolist())
    assert (got[a == 0] == 0).all()
    print(f"{channels} channel(s): worst error / bound = {(err[a > 0] / bound[a > 0]).max():.3f}, up to {int(m.max())} notes on a sample")


@pytest.mark.parametrize("channels", [1, 2])
def test_crowded_curves(dense, channels):
    """The kernel keeps 256 points of the current curve around its tile in LDS and reads global memory when a tile needs more.  Curve 0
    has a point on every sample from 4000 to 4700: the first tile's window covers it, the second tile needs 606 points and takes the
    other path, the third lies behind the last point.  Curve 1 has a point every 17 samples, 241 a tile: the window covers every tile."""
    rng = np.random.default_rng(5)
    crowded = [(pos, float(np.float32(l)), float(np.float32(r))) for pos, (l, r) in zip(range(4000, 4701), rng.random((701, 2)))]
    spaced = [(pos, float(np.float32(l)), float(np.float32(r))) for pos, (l, r) in zip(range(3, TOTAL, 17), rng.random((TOTAL, 2)))]
    points, first = crowded + spaced, [0, len(crowded), len(crowded) + len(spaced)]
    table = [row[:5] + (n % 2,) for n, row in enumerate(dense["table"])]
    got, _, _ = _raw(dense["waves"], table, points, first, TOTAL, channels)
    assert np.array_equal(got.cpu().numpy(), CRF.mix_f32(dense["host"], table, points, first, TOTAL, channels))


def test_constant_curves_give_the_plain_mixes(dense):
    """Every curve the one point (0, 1, 1): gs_note_mix_stereo's bits with gain_l = gain_r = gain, gs_note_mix's with one channel --
    the mix, the peak, the normalised clip and the PCM."""
    K = _K()
    waves, table = dense["waves"], dense["table"]
    stereo_table = [row[:5] + (row[4],) for row in table]
    for normalize in (False, True):
        want, want_pcm, want_peak = K.note_mix_stereo(waves, stereo_table, TOTAL, normalize=normalize, want_pcm=True)
        got, pcm, peak = _raw(waves, table, ONES, ONES_FIRST, TOTAL, 2, normalize=normalize, want_pcm=True)
        assert torch.equal(got, want) and torch.equal(pcm, want_pcm) and torch.equal(peak, want_peak)
        want, want_pcm, want_peak = K.note_mix(waves, [row[:5] for row in table], TOTAL, normalize=normalize, want_pcm=True)
        got, pcm, peak = _raw(waves, table, ONES, ONES_FIRST, TOTAL, 1, normalize=normalize, want_pcm=True)
        assert torch.equal(got[0], want) and torch.equal(pcm[:, 0], want_pcm) and torch.equal(peak, want_peak)
    assert float(want_peak) > 1.0


@pytest.mark.parametrize("channels", [1, 2])
def test_finish_stage(dense, channels):
    waves, table, points, first = dense["waves"], dense["table"], dense["points"], dense["first"]
    mix = dense[channels]["mix"].cpu().numpy()
    assert np.abs(mix).max() > 1.0
    out, pcm, peak = _raw(waves, table, points, first, TOTAL, channels, normalize=True, want_pcm=True)
    if channels == 2:
        want_peak, want, want_pcm = STR.finish(mix, True)
    else:
        want_peak = np.float32(np.abs(mix).max())
        want = (mix.astype(np.float64) / np.float64(want_peak)).astype(np.float32)
        want_pcm = SRF.pcm16(want).T
    assert float(peak) == float(want_peak) and np.array_equal(out.cpu().numpy(), want) and np.array_equal(pcm.cpu().numpy(), want_pcm)
    plain, pcm, _ = _raw(waves, table, points, first, TOTAL, channels, normalize=False, want_pcm=True)
    assert torch.equal(plain, dense[channels]["mix"]) and np.array_equal(pcm.cpu().numpy(), SRF.pcm16(mix).T)
    # through the Python layer: the same three results, in note_mix's / note_mix_stereo's shapes
    out2, pcm2, peak2 = _K().note_mix_curves(waves, table, points, first, TOTAL, channels=channels, normalize=True, want_pcm=True)
    assert out2.shape == ((2, TOTAL) if channels == 2 else (TOTAL,)) and pcm2.shape == ((TOTAL, 2) if channels == 2 else (TOTAL,))
    assert torch.equal(out2.reshape(channels, TOTAL), out) and torch.equal(pcm2.reshape(TOTAL, channels), pcm.new_tensor(want_pcm)) and torch.equal(peak2, peak)


@pytest.mark.parametrize("channels", [1, 2])
def test_store_paths(dense, channels):
    waves, table, points, first = dense["waves"], dense["table"], dense["points"], dense["first"]
    out, pcm, peak = _raw(waves, table, points, first, TOTAL, channels, normalize=True, want_pcm=True)
    off = _raw(waves, table, points, first, TOTAL, channels, normalize=True, want_pcm=True, offset=1)      # out off 16 bytes: sample by sample
    assert off[0].data_ptr() % 16 == 4 and out.data_ptr() % 16 == 0
    assert torch.equal(off[0], out) and torch.equal(off[1], pcm) and torch.equal(off[2], peak)
    assert torch.equal(_raw(waves, table, points, first, TOTAL, channels, offset=1)[0], dense[channels]["mix"])


def test_a_note_with_a_curve_out_of_range_is_skipped():
    """curve = n_curves and curve = -1 among valid notes, handed to the entry point itself: the kernel judges the note before it reads
    `first` for it, and every index into `points` is clamped, so the call succeeds and the result is the mix of the valid notes bit for
    bit, with nothing around out and pcm written (_raw checks the sentinels).  Nothing here can fault: that is the point."""
    waves = (torch.rand(4, L, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    good = [(10, 400, 100, 0, 0.9, 0), (300, L, 0, 1, 0.7, 1), (350, 20, 160, 2, 1.0, 0), (900, 700, 160, 3, 0.4, 1), (1500, 64, 64, 0, 0.2, 1)]
    points, first = [(0, 1.0, 0.2), (800, 0.1, 0.9), (1200, 0.5, 0.5), (400, 0.3, 0.6)], [0, 3, 4]
    total = 1700
    table = sorted(good + [(340, 500, 160, 2, 0.8, 2), (360, 500, 160, 2, 0.8, -1)], key=lambda n: n[0])
    for channels in (1, 2):
        out, pcm, peak = _raw(waves, table, points, first, total, channels, normalize=True, want_pcm=True)
        want, want_pcm, want_peak = _raw(waves, good, points, first, total, channels, normalize=True, want_pcm=True)
        assert torch.equal(out, want) and torch.equal(pcm, want_pcm) and torch.equal(peak, want_peak) and float(peak) > 0
        assert np.array_equal(_raw(waves, table, points, first, total, channels)[0].cpu().numpy(),
                              CRF.mix_f32(waves.cpu().numpy(), good, points, first, total, channels))
    with pytest.raises(ValueError, match="note_mix_curves: note . field 'curve'"):
        _K().note_mix_curves(waves, table, points, first, total)


def test_refusals_launch_nothing():
    """Every GS_ERR_ARG case of tests/test_controllers_cpu.py with real buffers behind the pointers: the code, a message, and out as it was."""
    from gansynth_amd import _lib
    from tests.test_controllers_cpu import REFUSALS
    K = _K()
    waves = torch.zeros(4, 1024, device="cuda")
    notes = _upload((_lib.GsMixNoteCurve * 3)(*[_lib.GsMixNoteCurve(0, 10, 0, 0, 1.0, 0, 0)] * 3))
    pts = _upload((_lib.GsCurvePoint * 5)(*[_lib.GsCurvePoint(i, 1.0, 1.0) for i in range(5)]))
    firsts = torch.tensor([0, 2, 5], dtype=torch.int32, device="cuda")
    out = torch.full((2, 5000), SENTINEL, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    good = dict(waves=waves.data_ptr(), rows=4, length=1024, row_stride=1024, notes=notes.data_ptr(), n_notes=3, points=pts.data_ptr(), n_points=5,
                first=firsts.data_ptr(), n_curves=2, channels=2, total=5000, normalize=1, out=out.data_ptr(), out_stride=5000, pcm=None, peak=None,
                ws=ws.data_ptr(), ws_bytes=1 << 20, stream=None)
    for field, value, message in REFUSALS:
        if isinstance(value, int) and value >= 0x10000:            # a misaligned pointer: the real one moved by as much
            value = (ws.data_ptr() if good[field] is None else good[field]) + (value - 0x10000)
        assert K.lib.gs_note_mix_curves(*dict(good, **{field: value}).values()) == -1, (field, value)
        assert message in K.lib.gs_last_error() and b"note_mix_curves" in K.lib.gs_last_error(), (field, value, K.lib.gs_last_error())
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------- end to end
def _performance_file():
    """Format 1, 960 ticks a second, two channels, five notes (one more outside the label table): a pedal on channel 1 that holds the first
    note to tick 40, an expression ramp on channel 1 and a pan on channel 2 in the middle of a note."""
    conductor = track([(0, tempo(500000)), (0, END)])
    one = track([
        (0, [0xB0, 7, 110]),       # tick 0    volume 110: set-up, no ramp
        (0, [0x90, 60, 100]),      #           A on
        (5, [0xB0, 64, 127]),      # tick 5    pedal down
        (15, [0x80, 60, 0]),       # tick 20   A off under the pedal: held to tick 40
        (0, [0xB0, 11, 40]),       #           expression down ...
        (10, [0x90, 67, 90]),      # tick 30   B on
        (2, [0xB0, 11, 120]),      # tick 32   ... and up again, in the middle of B
        (8, [0xB0, 64, 0]),        # tick 40   pedal up
        (20, [0x80, 67, 0]),       # tick 60   B off
        (0, [0x90, 100, 9]),       #           not in the label table: dropped
        (10, [0x80, 100, 0]),
        (30, [0x90, 72, 127]),     # tick 100  C on
        (30, [0x80, 72, 0]),       # tick 130
        (0, END)])
    two = track([
        (0, [0xC1, 33]),
        (0, [0xB1, 10, 20]),       # tick 0    pan left: set-up
        (10, [0x91, 48, 80]),      # tick 10   D on
        (15, [0xB1, 10, 110]),     # tick 25   pan to the right in the middle of D
        (25, [0x81, 48, 0]),       # tick 50   D off
        (40, [0x91, 50, 70]),      # tick 90   E on
        (5, [0xB1, 7, 60]),        # tick 95   volume down in the middle of E
        (35, [0x81, 50, 0]),       # tick 130
        (0, END)])
    return header(1, 3, 480) + conductor + one + two


KW = dict(batch_size=4, release_seconds=0.01, seconds_per_instrument=0.04, seed=2)


def test_synthesize_controllers_end_to_end(gpu_store):
    from gansynth_amd import notes as N
    from tests.test_ensemble_gpu import _hand_waves
    from tests.test_notes_gpu import _model
    K = _K()
    model = _model()
    data = _performance_file()
    before = model.synthesize(data, ensemble=True, stereo=True, spread=0.5, **KW)
    info = {}
    clip, pcm = model.synthesize(data, controllers=True, controller_ramp=0.001, ensemble=True, stereo=True, spread=0.5, normalize=False, want_pcm=True,
                                 info=info, **KW)
    assert info["controls"] == {"volume": 2, "expression": 2, "pan": 2} and info["pedal_extended"] == 1 and info["dropped"] == 1
    assert info["parts"] == [N.Part(0, 0), N.Part(1, 33)] and info["part_of_note"] == [0, 1, 0, 1, 0] and info["channels"] == 2
    # the rules by hand: (pitch, velocity, start, end) in ticks, A held by the pedal to tick 40
    def at(tick):   # the tempo map's own arithmetic: 500000 microseconds a quarter of 480 ticks
        return tick * 500000 / (480 * 1e6)

    notes = [(60, 100, 0.0, at(40)), (48, 80, at(10), at(50)), (67, 90, at(30), at(60)), (50, 70, at(90), at(130)), (72, 127, at(100), at(130))]
    assert [tuple(n) for n in info["notes"]] == notes
    table, total, _, _ = SRF.schedule(notes, range(24, 85), 16000, 1024, 0.01)
    controls = [[(0.0, "volume", 110), (at(20), "expression", 40), (at(32), "expression", 120)],
                [(0.0, "pan", (20 - 64) / 63), (at(25), "pan", (110 - 64) / 63), (at(95), "volume", 60)]]
    points, first = CRF.curves(controls, [0.0, 0.0], 16000, 0.001, True)      # (channel 2 is panned in the score: position 0; channel 1 alone: 0)
    assert info["total_samples"] == total and info["curve_points"] == len(points) and clip.shape == (2, total) and pcm.shape == (total, 2)
    waves = _hand_waves(model, info, 4)
    curve_table = [row + (part,) for row, part in zip(table, info["part_of_note"])]
    ref, a, m = CRF.mix(waves.cpu().numpy(), curve_table, points, first, total, 2)
    err = np.abs(clip.cpu().numpy().astype(np.float64) - ref)
    assert (err <= CRF.bound(a, m[None])).all() and float(clip.abs().max()) > 0 and info["peak"] == float(clip.abs().max())
    assert np.array_equal(clip.cpu().numpy(), CRF.mix_f32(waves.cpu().numpy(), curve_table, points, first, total, 2))
    assert np.array_equal(pcm.cpu().numpy(), SRF.pcm16(clip.cpu().numpy()).T)
    # one channel: the same curves' amplitudes without the pan
    mono_info = {}
    mono = model.synthesize(data, controllers=True, controller_ramp=0.001, ensemble=True, normalize=False, info=mono_info, **KW)
    mono_points, mono_first = CRF.curves(controls, [0.0, 0.0], 16000, 0.001, False)
    assert mono.shape == (total,) and mono_info["channels"] == 1 and torch.equal(mono_info["latents"], info["latents"])
    assert np.array_equal(mono.cpu().numpy(), CRF.mix_f32(waves.cpu().numpy(), curve_table, mono_points, mono_first, total, 1)[0])
    # without the flag: the path as it was -- read_score's notes (A ends at tick 20), schedule_gains' table, ONE gs_note_mix_stereo call
    plain_info = {}
    after = model.synthesize(data, ensemble=True, stereo=True, spread=0.5, info=plain_info, **KW)
    score = N.read_score(data)
    index = N.kept_indices(score.notes, range(24, 85))
    kept, plain_table, plain_total, _ = N.schedule(score.notes, range(24, 85), 16000, 1024, 0.01)
    assert kept[0].end == at(20) and "controls" not in plain_info and "pedal_extended" not in plain_info
    stereo_table = [row[:4] + g for row, g in zip(plain_table, N.schedule_gains(index, score, 0.5))]
    want, _, _ = K.note_mix_stereo(_hand_waves(model, plain_info, 4), stereo_table, plain_total, normalize=True)
    assert torch.equal(after, want) and torch.equal(after, before)


def test_set_up_controllers_agree_with_the_note_gains(gpu_store):
    """Every controller at tick 0: controllers=True and ensemble=True, stereo=True give the same gains to the same samples, through
    differently rounded products -- they agree within the sum of the two bounds."""
    from tests.test_ensemble_gpu import _hand_waves
    from tests.test_notes_gpu import _model
    from gansynth_amd import notes as N
    model = _model()
    one = track([(0, [0xB0, 7, 90]), (0, [0xB0, 10, 30]), (0, [0x90, 60, 100]), (30, [0x80, 60, 0]), (10, [0x90, 64, 50]), (40, [0x80, 64, 0]), (0, END)])
    two = track([(0, [0xB1, 7, 120]), (0, [0xB1, 10, 100]), (5, [0x91, 55, 80]), (50, [0x81, 55, 0]), (0, END)])
    data = header(1, 2, 480) + one + two
    info, plain_info = {}, {}
    got = model.synthesize(data, controllers=True, ensemble=True, stereo=True, normalize=False, info=info, **KW)
    plain = model.synthesize(data, ensemble=True, stereo=True, normalize=False, info=plain_info, **KW)
    assert info["curve_points"] == 2 and info["controls"] == {"volume": 2, "expression": 0, "pan": 2} and info["notes"] == plain_info["notes"]
    assert torch.equal(info["latents"], plain_info["latents"])
    waves = _hand_waves(model, info, 4).cpu().numpy()
    score = N.read_score(data)
    index = N.kept_indices(score.notes, range(24, 85))
    _, table, total, _ = N.schedule(score.notes, range(24, 85), 16000, 1024, 0.01)
    _, a_plain, m = STR.mix(waves, [row[:4] + g for row, g in zip(table, N.schedule_gains(index, score, 0.0))], total)
    points, first = CRF.curves([[(0.0, "volume", 90), (0.0, "pan", (30 - 64) / 63)], [(0.0, "volume", 120), (0.0, "pan", (100 - 64) / 63)]],
                               [0.0, 0.0], 16000, 0.01, True)
    _, a_curves, _ = CRF.mix(waves, [row + (score.part[i],) for row, i in zip(table, index)], points, first, total, 2)
    diff = np.abs(got.cpu().numpy().astype(np.float64) - plain.cpu().numpy().astype(np.float64))
    assert (diff <= CRF.bound(a_curves, m[None]) + SRF.bound(a_plain, m[None])).all() and float(got.abs().max()) > 0


def test_driver_with_controllers(gpu_store, tmp_path):
    """What `gan_synth_main.py --synthesize score.mid --ensemble --stereo --controllers --controller_ramp 0.001` runs after building its model."""
    from scipy.io import wavfile
    import gan_synth_main as main
    from tests.test_notes_gpu import _model
    model = _model()
    (tmp_path / "score.mid").write_bytes(_performance_file())
    argv = ["--synthesize", str(tmp_path / "score.mid"), "--output", str(tmp_path / "x.wav"), "--batch_size", "4", "--release_seconds", "0.01",
            "--model_dir", str(tmp_path / "no_model"), "--ensemble", "--stereo"]
    lines = []
    info = main.synthesize_to_wav(model, main.parser.parse_args(argv + ["--controllers", "--controller_ramp", "0.001"]), range(24, 85), log=lines.append)
    rate, data = wavfile.read(str(tmp_path / "x.wav"))
    assert rate == 16000 and data.shape == (info["total_samples"], 2) and info["pedal_extended"] == 1
    _, pcm = model.synthesize(str(tmp_path / "score.mid"), want_pcm=True, batch_size=4, release_seconds=0.01, ensemble=True, stereo=True,
                              controllers=True, controller_ramp=0.001)
    assert np.array_equal(data, pcm.cpu().numpy()) and np.abs(data).max() > 0
    assert "5 notes kept, 1 dropped" in lines[-2]
    assert lines[-1] == "controllers: 2 volume, 2 expression and 2 pan events in 10 curve points, 1 notes held by the pedal"
    # without the flag the driver's call and its summary are what they were
    plain = []
    plain_info = main.synthesize_to_wav(model, main.parser.parse_args(argv), range(24, 85), log=plain.append)
    assert "controls" not in plain_info and not any(line.startswith("controllers:") for line in plain)
