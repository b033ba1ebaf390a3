"""GPU: gs_note_warp against tests/bend_ref.py -- every case of bend_ref.cases() within four times the error of the fp32 restatement
(tests/test_bend_cpu.py::test_fp32_restatement_on_the_gpu_cases has those figures without a device), bit for bit where the rule is exact,
untouched sentinels around every destination, bad tables that the kernel must skip or clamp, kernels.note_warp's refusals, and
GANSynth.synthesize(bend=...) end to end on the reduced PGGAN of tests/test_notes_gpu.py."""
import numpy as np
import pytest
import torch

from tests import bend_ref as B
from tests.test_bend_cpu import BAD_NOTES, REFUSALS, bend
from tests.test_notes_cpu import END, header, track

pytestmark = pytest.mark.gpu
PAD = 64
MARGIN = 4      # the project's margin between a kernel and the fp32 restatement of its rule (tests/test_loudness_gpu.py)


def _K():
    from gansynth_amd import kernels
    return kernels.get()


def _upload(arr):
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _buffer(x):
    """[ROWS, LENGTH] with rows STRIDE apart inside a buffer of sentinels: row SRC holds x, rows 0 and 2 and the stride padding of the
    source rows are NaN, everything else -- the destination rows, the guard row between them, the pads -- is the sentinel."""
    buf = torch.full((PAD + B.ROWS * B.STRIDE + PAD,), B.SENTINEL, dtype=torch.float32)
    rows = buf[PAD:PAD + B.ROWS * B.STRIDE].view(B.ROWS, B.STRIDE)
    rows[0] = rows[2] = float("nan")
    rows[B.SRC] = float("nan")
    rows[B.SRC, :B.LENGTH] = torch.from_numpy(x)
    return buf.cuda()


def _raw(x, points, first, notes):
    """gs_note_warp itself on the tables AS GIVEN (no validation), on _buffer(x) -> the whole buffer on the host, after checking that the
    call succeeded (_check_untouched then looks at everything around what should have been written)."""
    from gansynth_amd import _lib, kernels
    K = _K()
    buf = _buffer(x)
    rows = buf[PAD:PAD + B.ROWS * B.STRIDE].view(B.ROWS, B.STRIDE)
    nts = _upload((_lib.GsWarpNote * len(notes))(*[_lib.GsWarpNote(*[int(v) for v in note]) for note in notes]))
    pts = _upload((_lib.GsWarpPoint * len(points))(*[_lib.GsWarpPoint(float(p), float(r), float(c)) for p, r, c in points]))
    firsts = torch.tensor(first, dtype=torch.int32, device="cuda")
    code = K.lib.gs_note_warp(rows.data_ptr(), B.ROWS, B.LENGTH, B.STRIDE, nts.data_ptr(), len(notes), pts.data_ptr(), firsts.data_ptr(),
                              len(first) - 1, len(points),
                              K.note_warp_table_dev("cuda").data_ptr(), kernels._stream())
    torch.cuda.synchronize()
    assert code == 0, K.lib.gs_last_error()
    return buf.cpu().numpy()


def _check_untouched(buf, x, written):
    """`written`: dst_row -> count.  Everything else is as _buffer left it."""
    want = _buffer(x).cpu().numpy()
    rows, want_rows = (b[PAD:PAD + B.ROWS * B.STRIDE].reshape(B.ROWS, B.STRIDE) for b in (buf, want))
    assert np.array_equal(buf[:PAD], want[:PAD]) and np.array_equal(buf[-PAD:], want[-PAD:])
    for r in range(B.ROWS):
        lo = written.get(r, 0)
        assert np.array_equal(rows[r, lo:], want_rows[r, lo:], equal_nan=True), r
    return rows


@pytest.fixture(scope="module")
def source():
    return B.source()


@pytest.fixture(scope="module")
def reference(source):
    """bend_ref's cases through the restatement, once: name -> [(warp_f32, warp_f64, B)] per note."""
    return {name: B.run_case(source, case, "f32") for name, case in B.cases().items()}


@pytest.mark.parametrize("name", list(B.cases()))
def test_cases_against_the_restatement(source, reference, name):
    points, first, notes = B.cases()[name]
    rows = _check_untouched(_raw(source, points, first, notes), source, {dst: count for _, dst, _, count, _ in notes})
    got = np.concatenate([rows[dst, :count] for _, dst, _, count, _ in notes])
    z32, y64, bound = (np.concatenate([r[i] for r in reference[name]]) for i in range(3))
    e_kernel, e_f32 = B.error_ratio(got, y64, bound), B.error_ratio(z32, y64, bound)
    print(f"{name}: e(kernel) = {e_kernel:.3g}, e(warp_f32) = {e_f32:.3g}, ratio {e_kernel / e_f32 if e_f32 else 0:.2f}")
    assert np.isfinite(got).all() and e_kernel <= MARGIN * e_f32, (name, e_kernel, e_f32)
    if name == "ratio 1":                                  # every coefficient but one an exact 0: the row comes back unchanged
        assert np.array_equal(got.view(np.uint32), source.view(np.uint32))
    if name == "ratio 4":                                  # bent up: out of waveform early, exact zeros to the end
        assert (got[B.LENGTH // 4 + B.HALF:] == 0).all() and np.abs(got[:700]).max() > 0.1


def test_an_impulse_returns_the_coefficients_bit_for_bit():
    """An impulse at sample s under the constant ratio 0.5: output k is the coefficient of tap s at position k / 2 -- the table's entries
    at offsets of whole and half samples --, which pins lead and lag."""
    s = 700
    x = np.zeros(B.LENGTH, dtype=np.float32)
    x[s] = 1.0
    points = B.with_cum([(0, 0.5)])
    rows = _check_untouched(_raw(x, points, [0, 1], [(B.SRC, B.DST, 0, B.LENGTH, 0)]), x, {B.DST: B.LENGTH})
    n, f, c = B.positions(points, 0, B.LENGTH)
    want = B.warp_f32(x, n, f, c)
    assert np.array_equal(rows[B.DST, :B.LENGTH].view(np.uint32), want.view(np.uint32))
    T = B.table()
    assert want[2 * s] == 1.0 and want[2 * s + 1] == T[B.Q // 2] and want[2 * s - 1] == T[B.Q // 2] and want[2 * s + 3] == T[3 * B.Q // 2]
    assert np.count_nonzero(want) == 1 + 2 * B.Z          # the centre and the 2 Z half-sample offsets inside the window


def test_two_calls_are_bit_identical(source):
    points, first, notes = B.cases()["a point every 2 samples"]
    a, b = _raw(source, points, first, notes), _raw(source, points, first, notes)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ robustness
def test_bad_tables_are_skipped_or_clamped(source):
    """Bad tables handed to the entry point itself.  Nothing here can fault: every bad entry is one that the kernel judges or clamps
    before it forms an address, which is the point.  The valid note's row is bit for bit what a call without the bad entries writes, and
    nothing else is touched."""
    good_points = B.with_cum([(0, 1.0), (700, 1.2), (2500, 0.95)])
    good = (B.SRC, B.DST, 100, 2500, 0)
    want = _check_untouched(_raw(source, good_points, [0, 3], [good]), source, {B.DST: 2500})
    # notes the kernel skips: their destination stays a row of sentinels
    skipped = [(-1, B.DST_B, 0, 100, 0), (B.ROWS, B.DST_B, 0, 100, 0), (B.SRC, B.ROWS, 0, 100, 0), (B.SRC, -1, 0, 100, 0), (B.SRC, B.DST_B, 0, 0, 0),
               (B.SRC, B.DST_B, 0, B.LENGTH + 1, 0), (B.SRC, B.DST_B, -1, 100, 0), (B.SRC, B.DST_B, 0, 100, 1), (B.SRC, B.DST_B, 0, 100, -1),
               (B.DST_B, B.DST_B, 0, 100, 0), (2 ** 31 - 1, B.DST_B, 0, 100, 0), (B.SRC, B.DST_B, 0, -(2 ** 31), 0)]
    rows = _check_untouched(_raw(source, good_points, [0, 3], skipped[:6] + [good] + skipped[6:]), source, {B.DST: 2500})
    assert np.array_equal(rows.view(np.uint32), want.view(np.uint32))
    # `first` out of range: clamped into [0, n_points), which here is what the well-formed table says
    for first in ([-7, 3], [0, 99999], [-2 ** 31, 2 ** 31 - 1]):
        rows = _check_untouched(_raw(source, good_points, first, [good]), source, {B.DST: 2500})
        assert np.array_equal(rows.view(np.uint32), want.view(np.uint32)), first
    # a second curve that is bad in itself, named by a second note: that note's row holds whatever the clamped curve gives (its count
    # samples are written, nothing beyond), the valid note is untouched by it
    other = (B.SRC, B.DST_B, 40, 2000, 1)
    for bad in ([(500.0, 1.0, 500.0), (500.0, 2.0, 500.0), (400.0, 1.5, 300.0)],                     # segments of length 0 and below
                [(0.0, float("nan"), 0.0), (1000.0, 100.0, 900.0), (2000.0, -3.0, 2000.0)],          # ratios: NaN, too large, negative
                [(0.0, 1.0, float("nan")), (1000.0, 1.0, 1e300), (1500.0, 1.0, -1e300), (2500.0, 1.0, float("inf"))],   # positions anywhere
                [(0.0, 1.0, 0.0), (1000.0, 1.0, 5e6), (1001.0, 1.0, -5e6)]):                          # q far outside the row, both ways
        rows = _check_untouched(_raw(source, good_points + bad, [0, 3, 3 + len(bad)], [good, other]), source, {B.DST: 2500, B.DST_B: 2000})
        assert np.array_equal(rows[B.DST].view(np.uint32), want[B.DST].view(np.uint32))
        assert not (rows[B.DST_B, :2000] == B.SENTINEL).any()


def test_note_warp_refuses_bad_tables(source):
    K = _K()
    waves = torch.zeros(4, 1024, device="cuda")
    from tests.test_bend_cpu import GOOD_FIRST, GOOD_NOTES, GOOD_POINTS
    for bad, message in BAD_NOTES:
        with pytest.raises(ValueError, match="note_warp: " + message):
            K.note_warp(waves, [bad, GOOD_NOTES[1]], GOOD_POINTS, GOOD_FIRST)
    with pytest.raises(ValueError, match="note_warp: waves must be"):
        K.note_warp(waves.double(), GOOD_NOTES, GOOD_POINTS, GOOD_FIRST)
    with pytest.raises(ValueError, match="note_warp: the rows of waves"):
        K.note_warp(waves.t(), GOOD_NOTES, GOOD_POINTS, GOOD_FIRST)
    assert (waves == 0).all()
    # through the Python layer: the table is uploaded once per device, the rows written in place
    waves = torch.zeros(B.ROWS, B.LENGTH, device="cuda")
    waves[B.SRC] = torch.from_numpy(source).cuda()
    points, first, notes = B.cases()["two notes on one curve"]
    table = K.note_warp_table_dev("cuda")
    assert K.note_warp(waves, notes, points, first) is waves and K.note_warp_table_dev("cuda") is table
    want = _raw(source, points, first, notes)[PAD:PAD + B.ROWS * B.STRIDE].reshape(B.ROWS, B.STRIDE)
    for _, dst, _, count, _ in notes:
        assert np.array_equal(waves[dst, :count].cpu().numpy(), want[dst, :count]) and (waves[dst, count:] == 0).all()


def test_refusals_launch_nothing():
    """Every GS_ERR_ARG case of tests/test_bend_cpu.py with real buffers behind the pointers: the code, a message, and waves as they were."""
    from gansynth_amd import _lib
    K = _K()
    waves = torch.full((4, 1024), B.SENTINEL, device="cuda")
    notes = _upload((_lib.GsWarpNote * 2)(_lib.GsWarpNote(0, 2, 0, 100, 0), _lib.GsWarpNote(1, 3, 0, 100, 1)))
    pts = _upload((_lib.GsWarpPoint * 3)(*[_lib.GsWarpPoint(float(i), 1.5, 1.5 * i) for i in range(3)]))
    firsts = torch.tensor([0, 2, 3], dtype=torch.int32, device="cuda")
    good = dict(waves=waves.data_ptr(), rows=4, length=1024, row_stride=1024, notes=notes.data_ptr(), n_notes=2, points=pts.data_ptr(),
                first=firsts.data_ptr(), n_curves=2, n_points=3, table=K.note_warp_table_dev("cuda").data_ptr(), stream=None)
    for field, value, message in REFUSALS:
        if isinstance(value, int) and value >= 0x10000 and field in ("waves", "notes", "points", "first", "table"):   # the real pointer, moved
            value = good[field] + (value - 0x10000)
        assert K.lib.gs_note_warp(*dict(good, **{field: value}).values()) == -1, (field, value)
        assert message in K.lib.gs_last_error() and b"note_warp" in K.lib.gs_last_error(), (field, value, K.lib.gs_last_error())
    torch.cuda.synchronize()
    assert (waves == B.SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------- end to end
KW = dict(batch_size=4, release_seconds=0.01, seconds_per_instrument=0.04, seed=2)


def _bent_score():
    """Format 1, 960 ticks a second, two channels, five notes in the label table: channel 1 bends up a semitone in the middle of its
    first note and back before its second ends; channel 2 (program 33) sets a range of 12 and never bends."""
    one = track([
        (0, [0x90, 60, 100]),        # tick 0    A on
        (20, [0xE0] + bend(4096)),   # tick 20   up a semitone (range 2) in the middle of A
        (20, [0x80, 60, 0]),         # tick 40   A off
        (10, [0x90, 67, 90]),        # tick 50   B on, still bent
        (10, [0xE0] + bend(0)),      # tick 60   back in the middle of B
        (10, [0x80, 67, 0]),         # tick 70   B off
        (30, [0x90, 72, 127]),       # tick 100  C on: the bend is over
        (30, [0x80, 72, 0]),         # tick 130
        (0, END)])
    two = track([
        (0, [0xC1, 33]), (0, [0xB1, 101, 0]), (0, [0xB1, 100, 0]), (0, [0xB1, 6, 12]), (0, [0xB1, 10, 100]),
        (10, [0x91, 48, 80]),        # tick 10   D on
        (40, [0x81, 48, 0]),         # tick 50
        (40, [0x91, 50, 70]),        # tick 90   E on
        (40, [0x81, 50, 0]),         # tick 130
        (0, END)])
    return header(1, 2, 480) + one + two


def _plain_score():
    return header(1, 1, 480) + track([(0, [0xB0, 101, 0]), (0, [0xB0, 100, 0]), (0, [0xB0, 6, 12]), (0, [0x90, 60, 100]), (30, [0x80, 60, 0]),
                                      (10, [0x90, 64, 50]), (40, [0x80, 64, 0]), (0, END)])


def test_bend_on_a_score_without_bends_changes_nothing(gpu_store):
    from tests.test_notes_gpu import _model
    K = _K()
    model = _model()
    for data in (_plain_score(), _performance_bytes()):
        for how in (dict(), dict(ensemble=True, stereo=True, spread=0.5), dict(controllers=True, stereo=True)):
            launches = K.note_warps
            want, want_pcm = model.synthesize(data, want_pcm=True, **how, **KW)
            info = {}
            got, pcm = model.synthesize(data, want_pcm=True, bend=True, info=info, **how, **KW)
            assert torch.equal(got, want) and torch.equal(pcm, want_pcm) and K.note_warps == launches
            # (the range set-up of _plain_score is an event -- a target of 0 semitones -- and bends no note)
            assert info["bent_notes"] == 0 and sum(info["bends"]) == (1 if data == _plain_score() else 0)


def _performance_bytes():
    from tests.test_controllers_gpu import _performance_file
    return _performance_file()


def test_a_bent_score_is_note_mix_over_note_warp(gpu_store):
    from gansynth_amd import notes as N
    from tests.test_ensemble_gpu import _hand_waves
    from tests.test_notes_gpu import _model
    K = _K()
    model = _model()
    data = _bent_score()
    info = {}
    launches = K.note_warps
    clip, pcm = model.synthesize(data, bend=True, controller_ramp=0.001, want_pcm=True, info=info, **KW)
    assert K.note_warps == launches + 1
    at = lambda tick: tick * 500000 / (480 * 1e6)
    bends = [[(at(20), 1.0), (at(60), 0.0)], [(0.0, 0.0)]]
    assert N.read_bends(data) == bends and info["bends"] == [2, 1]
    points, first = B.curves(bends, 16000, 0.001)
    assert info["bend_points"] == len(points) == 6 and first == [0, 5, 6] and info["bent_notes"] == 2            # A and B; C, D and E are not touched
    score = N.read_score(data)
    kept, table, total, _ = N.schedule(score.notes, range(24, 85), 16000, 1024, 0.01)
    assert [n.pitch for n in kept] == [60, 48, 67, 50, 72] and info["total_samples"] == total
    # by hand: the generated rows, two more rows for A (row 0) and B (row 2) on the curve of part 0, and the plain mix over them
    waves = torch.cat([_hand_waves(model, info, 4), torch.full((2, 1024), float("nan"), device="cuda")])
    warp_notes = [(0, 5, table[0][0], table[0][1] + table[0][2], 0), (2, 6, table[2][0], table[2][1] + table[2][2], 0)]
    K.note_warp(waves, warp_notes, points, first)
    by_hand = [row[:3] + (5 if n == 0 else 6 if n == 2 else row[3],) + row[4:] for n, row in enumerate(table)]
    want, want_pcm, _ = K.note_mix(waves, by_hand, total, normalize=True, want_pcm=True)
    assert torch.equal(clip, want) and torch.equal(pcm, want_pcm)
    # the bent rows are the restatement's, within the kernel's margin; and the clip differs from the unbent one where A and B sound
    src = waves[0].cpu().numpy()
    n, f, c = B.positions(points[first[0]:first[1]], warp_notes[0][2], warp_notes[0][3])
    y64, bound = B.warp_f64(src, n, f, c, want_bound=True)
    e32 = B.error_ratio(B.warp_f32(src, n, f, c), y64, bound)
    assert B.error_ratio(waves[5, :warp_notes[0][3]].cpu().numpy(), y64, bound) <= MARGIN * e32
    plain = model.synthesize(data, **KW)
    assert plain.shape == clip.shape and not torch.equal(plain, clip)


def test_bend_composes_with_stereo_controllers_and_the_output_rate(gpu_store):
    from tests.test_notes_gpu import _model
    model = _model()
    info = {}
    clip, pcm = model.synthesize(_bent_score(), bend=True, stereo=True, controllers=True, ensemble=True, sample_rate=48000, controller_ramp=0.001,
                                 want_pcm=True, info=info, **KW)
    n = info["output_samples"]
    assert clip.shape == (2, n) and pcm.shape == (n, 2) and pcm.dtype == torch.int16 and info["sample_rate"] == 48000
    assert info["bent_notes"] == 2 and info["bends"] == [2, 1] and info["channels"] == 2 and info["controls"] == {"volume": 0, "expression": 0, "pan": 1}
    assert int(pcm.abs().max()) <= 32767 and int(pcm.abs().max()) > 0 and torch.isfinite(clip).all() and float(clip.abs().max()) <= 1.0
    # the bends given by hand, per part, to a score that carries none: the same clip
    from gansynth_amd import notes as N
    again = model.synthesize(N.read_performance(_bent_score()), bend=N.read_bends(_bent_score()), stereo=True, controllers=True, ensemble=True,
                             sample_rate=48000, controller_ramp=0.001, **KW)
    assert torch.equal(again, clip)
    with pytest.raises(ValueError, match="one list of events per part"):
        model.synthesize(_bent_score(), bend=[[(0.0, 1.0)]], **KW)


def test_a_train_step_after_a_bent_synthesize_is_the_same_step():
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
                model.synthesize(_bent_score(), bend=True, info=info, **KW)
                assert info["bent_notes"] == 2
            lat, lab, real = R.synthetic_batch(4, rank=1, image_shape=(2, 16, 128))
            d = torch.as_tensor(model.discriminator_step(cuda(lat), cuda(lab), cuda(real))).detach().clone()
            g = torch.as_tensor(model.generator_step(cuda(lat), cuda(lab))).detach().clone()
            losses.append((d, g, model.g_params.flat.clone(), model.d_params.flat.clone()))
    finally:
        variables._default = old
    for a, b in zip(*losses):
        assert torch.equal(a, b)


def test_driver_with_bend(gpu_store, tmp_path):
    """What `gan_synth_main.py --synthesize score.mid --bend` runs after building its model."""
    from scipy.io import wavfile
    import gan_synth_main as main
    from tests.test_notes_gpu import _model
    model = _model()
    (tmp_path / "score.mid").write_bytes(_bent_score())
    argv = ["--synthesize", str(tmp_path / "score.mid"), "--batch_size", "4", "--release_seconds", "0.01", "--model_dir", str(tmp_path / "no_model")]
    lines = []
    info = main.synthesize_to_wav(model, main.parser.parse_args(argv + ["--output", str(tmp_path / "bent.wav"), "--bend", "--controller_ramp", "0.001"]),
                                  range(24, 85), log=lines.append)
    assert lines[-1] == "bend: 3 events on 2 parts in 6 curve points, 2 notes bent" and info["bent_notes"] == 2
    plain_lines = []
    plain_info = main.synthesize_to_wav(model, main.parser.parse_args(argv + ["--output", str(tmp_path / "plain.wav")]), range(24, 85), log=plain_lines.append)
    assert "bent_notes" not in plain_info and not any(line.startswith("bend:") for line in plain_lines)
    rate, bent = wavfile.read(str(tmp_path / "bent.wav"))
    _, plain = wavfile.read(str(tmp_path / "plain.wav"))
    assert rate == 16000 and bent.shape == plain.shape == (info["total_samples"],) and not np.array_equal(bent, plain)
    # without the flag: byte for byte the file of the unchanged path
    _, pcm = model.synthesize(str(tmp_path / "score.mid"), want_pcm=True, batch_size=4, release_seconds=0.01)
    wavfile.write(str(tmp_path / "want.wav"), rate=16000, data=pcm.cpu().numpy())
    assert (tmp_path / "plain.wav").read_bytes() == (tmp_path / "want.wav").read_bytes()
