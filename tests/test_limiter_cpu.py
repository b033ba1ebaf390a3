"""CPU: the look-ahead limiter without a device -- the properties of its restatement (tests/limiter_ref.py) on random and adversarial clips,
that a window moved by one sample is caught at the tile seams, the host checks of kernels.limit_shapes and gansynth_amd.limiter, the
arithmetic of pre_gain and of W, the C ABI's refusals (never-dereferenced pointers, as tests/test_abi_cpu.py) and the driver's flags."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import limiter_ref as LR

C, D = LR.C, LR.D


def _spike_clip(n, positions, rows=1, height=1.5):
    x = np.zeros((rows, n), dtype=np.float32) + np.float32(0.25)
    for p in positions:
        x[0, p] = np.float32(height)
    return x


def _adversarial(W):
    n = 6 * W + 50
    return {
        "spike at 0": _spike_clip(n, [0]),
        "spike at n - 1": _spike_clip(n, [n - 1]),
        "two spikes W apart": _spike_clip(n, [2 * W + 3, 3 * W + 3]),
        "two spikes W + 1 apart": _spike_clip(n, [2 * W + 3, 3 * W + 4]),
        "plateau": np.concatenate([np.full((1, 2 * W + 7), 0.25), np.full((1, W + 9), 0.9), np.full((1, 3 * W + 34), 0.25)], axis=1).astype(np.float32),
        "random": LR.draw(n, 1, W, seed=11),
        "random stereo": LR.draw(n, 2, W, seed=12),
    }


@pytest.mark.parametrize("W", [1, 7, 64, 240])
def test_properties_of_the_restatement(W):
    for name, x in _adversarial(W).items():
        y = LR.pre(x, D)
        ref, f32 = LR.limit_f64(y, C, W), LR.limit_f32(y, C, W)
        n = y.shape[1]
        assert ref.m.shape == (n + W,) and ref.g.shape == (n,) and ref.out.shape == y.shape, name
        assert (ref.g <= ref.r * (1 + 1e-15)).all() and (ref.g > 0).all(), name                      # every term of the mean is <= r[t]
        assert (np.abs(ref.out) <= np.float64(C)).all() and (np.abs(f32.out) <= C).all(), name       # the guarantee, bit for bit in fp32
        quiet = LR.quiet(y, C, W)
        assert quiet.any() and np.array_equal(f32.out[:, quiet], y[:, quiet]), name                  # identity where quiet, bit for bit
        assert np.array_equal(ref.out[:, quiet], y[:, quiet].astype(np.float64)), name
        loud = np.abs(y).max(axis=0) > C
        assert loud.any() and (ref.g[loud] < 1).all(), name
        assert np.abs(f32.g - ref.g).max() < (W + 1) * 2.0 ** -23, name                              # a sum of W + 1 terms <= 1, sequential
        assert np.abs(f32.m - ref.m).max() <= 2.0 ** -25, name                                       # one rounding of a quotient below 1


def test_quiet_clip_is_the_scaled_clip():
    x = LR.draw(5000, 2, 64, seed=3) * np.float32(0.3)
    y = LR.pre(x, D)
    assert np.abs(y).max() <= C
    for W in (1, 64, 2048):
        ref, f32 = LR.limit_f64(y, C, W), LR.limit_f32(y, C, W)
        assert (ref.g == 1).all() and (f32.g == 1).all() and np.array_equal(f32.out, y)


@pytest.mark.parametrize("W", [1, 5, 64])
def test_single_spike_is_low_on_exactly_its_window(W):
    n, t = 4 * W + 20, 2 * W + 5
    y = LR.pre(_spike_clip(n, [t]), D)
    ref = LR.limit_f64(y, C, W)
    low = np.flatnonzero(ref.m < 1) - W                      # as sample numbers s
    assert np.array_equal(low, np.arange(t - W, t + 1))
    reduced = np.flatnonzero(ref.g < 1)
    assert np.array_equal(reduced, np.arange(t - W, t + W + 1))   # attack over W samples before the spike, release over W after it
    assert ref.g[t] == pytest.approx(float(ref.r[t]), rel=1e-15) and (np.diff(ref.g[t - W:t + 1]) < 0).all() and (np.diff(ref.g[t:t + W + 1]) > 0).all()
    for edge in (0, n - 1):                                  # a spike at either end: the windows are clipped, not wrapped
        ref = LR.limit_f64(LR.pre(_spike_clip(n, [edge]), D), C, W)
        assert np.array_equal(np.flatnonzero(ref.m < 1) - W, np.arange(edge - W, edge + 1))
        assert ref.g[edge] == pytest.approx(float(ref.r[edge]), rel=1e-15)


def test_joint_gain_on_two_rows():
    n, W = 900, 64
    x = _spike_clip(n, [300], rows=2)
    x[1] = np.float32(0.2) * np.sin(np.arange(n, dtype=np.float32))
    y = LR.pre(x, D)
    ref = LR.limit_f64(y, C, W)
    assert np.array_equal(ref.g, LR.limit_f64(y[:1], C, W).g)                 # row 1 never exceeds the ceiling: the gain is row 0's
    assert np.allclose(ref.out[1], ref.g * y[1], rtol=0, atol=0)              # ... and row 1 is scaled by it all the same
    assert (ref.out[1, 300 - W:300 + W + 1] != y[1, 300 - W:300 + W + 1]).any()
    swapped = LR.limit_f64(y[::-1], C, W)
    assert np.array_equal(swapped.g, ref.g) and np.array_equal(swapped.out, ref.out[::-1])


def test_a_nan_sample_disturbs_no_neighbour():
    n, W = 700, 64
    x = LR.draw(n, 2, W, seed=5)
    zeroed = x.copy()
    zeroed[0, 333] = 0
    x[0, 333] = np.nan
    a, b = LR.limit_f32(LR.pre(x, D), C, W), LR.limit_f32(LR.pre(zeroed, D), C, W)
    assert np.isnan(a.out[0, 333]) and np.array_equal(a.g, b.g)
    keep = np.ones((2, n), dtype=bool)
    keep[0, 333] = False
    assert np.array_equal(a.out[keep], b.out[keep]) and LR.pcm(a.out)[333, 0] == 0 and LR.peak(a.out) == LR.peak(b.out)


@pytest.mark.parametrize("W", [63, 240])
def test_a_window_moved_by_one_sample_fails_the_seam_cases(W):
    """The GPU test's measure on the GPU test's clips, applied to a restatement whose minimum looks one sample too far ahead or behind: far
    outside 4 times limit_f32's error, through the spikes at the seams alone."""
    n = 3 * LR.T + 5
    x = LR.draw(n, 2, W)
    y = LR.pre(x, D)
    ref, f32 = LR.limit_f64(y, C, W), LR.limit_f32(y, C, W)
    bound = LR.FACTOR * LR.out_error(f32.out, ref)
    seams = np.zeros(n, dtype=bool)
    for seam in range(LR.T, n, LR.T):
        seams[seam - W - 2:seam + W + 3] = True
    for shift in (-1, 1):
        moved = LR.limit_f64(y, C, W, window_shift=shift)
        wrong = np.abs(moved.out - ref.out)
        assert wrong[:, seams].max() > 100 * bound, (shift, wrong[:, seams].max(), bound)
        assert (moved.g > ref.r * (1 + 1e-12)).any()                    # a window that misses its own sample: only the clamp holds the spike


# ----------------------------------------------------------------------------------------------------------- the Python layer
def test_limit_shapes_refusals_name_the_argument():
    from gansynth_amd import kernels, _lib
    assert _lib.LIMIT_MAX_LOOKAHEAD == LR.MAX_W == 2048 and _lib.LIMIT_TILE == LR.T
    x = torch.zeros(2, 100)
    assert kernels.limit_shapes(x, 1.5, 0.9, 240) == (2, 100) and kernels.limit_shapes(x[0], 1.5, 1.0, 1) == (1, 100)
    assert kernels.limit_shapes(x, 1, 1, 2048) == (2, 100)
    bad = [((torch.zeros(3, 10), 1.0, 0.9, 8), "x must have 1 or 2 rows"), ((torch.zeros(0), 1.0, 0.9, 8), "x must be a non-empty"),
           ((torch.zeros(4, dtype=torch.float64), 1.0, 0.9, 8), "x must be a non-empty fp32"), ((np.zeros(4, np.float32), 1.0, 0.9, 8), "x must be"),
           ((torch.zeros(2, 2, 2), 1.0, 0.9, 8), "x must be"),
           ((x, 0.0, 0.9, 8), "pre_gain must be positive"), ((x, -1.0, 0.9, 8), "pre_gain must be positive"), ((x, float("inf"), 0.9, 8), "pre_gain must be a finite"),
           ((x, float("nan"), 0.9, 8), "pre_gain must be a finite"), ((x, 1e39, 0.9, 8), "pre_gain must be positive and finite in fp32"),
           ((x, 1e-50, 0.9, 8), "pre_gain must be positive and finite in fp32"), ((x, "1", 0.9, 8), "pre_gain must be a finite"),
           ((x, 1.0, 0.0, 8), "ceiling must be in"), ((x, 1.0, 1.0001, 8), "ceiling must be in"), ((x, 1.0, -0.5, 8), "ceiling must be in"),
           ((x, 1.0, float("nan"), 8), "ceiling must be a finite"), ((x, 1.0, True, 8), "ceiling must be a finite"),
           ((x, 1.0, 0.9, 0), "lookahead must be an integer"), ((x, 1.0, 0.9, 2049), "lookahead must be an integer"),
           ((x, 1.0, 0.9, 8.0), "lookahead must be an integer"), ((x, 1.0, 0.9, True), "lookahead must be an integer")]
    for args, message in bad:
        with pytest.raises(ValueError, match=message):
            kernels.limit_shapes(*args)
        with pytest.raises(ValueError, match=message):      # the module-level call refuses before it asks for a device
            kernels.limit(*args)


def test_limiter_design_arithmetic():
    from gansynth_amd import limiter
    assert limiter.MAX_LOOKAHEAD == 2048
    pre_gain, c, w = limiter.design(48000, ceiling_db=-1.0, drive_db=6.0, lookahead_seconds=0.005, peak=2.5)
    assert c == 10.0 ** (-1.0 / 20) and w == 240 and pre_gain == c * 10.0 ** (6.0 / 20) / 2.5
    # drive 0: the peak lands exactly on the ceiling, the gain is 1 throughout
    pre_gain, c, w = limiter.design(16000, ceiling_db=-3.0, drive_db=0.0, peak=4.0)
    assert pre_gain == c / 4.0 and w == 80
    y = LR.pre(LR.draw(600, 2, 80, seed=9), 1.0)
    y = y / np.abs(y).max() * np.float32(4.0)
    peak = float(np.abs(y).max())
    pre_gain, c, w = limiter.design(16000, ceiling_db=-3.0, drive_db=0.0, peak=peak)
    scaled = LR.pre(y, pre_gain)
    f32 = LR.limit_f32(scaled, np.float32(c), w)
    assert np.abs(scaled).max() <= np.float32(c) and np.float32(c) - np.abs(scaled).max() <= 2.0 ** -22 and (f32.g == 1).all()
    for peak in np.random.Generator(np.random.PCG64(4)).uniform(0.01, 30.0, 200).astype(np.float32):      # whatever the peak, never past the ceiling
        pre_gain, c, _ = limiter.design(48000, ceiling_db=-1.0, drive_db=0.0, peak=float(peak))
        assert np.float32(np.float32(pre_gain) * peak) <= np.float32(c) and abs(pre_gain * float(peak) / c - 1) < 3e-7
    # a silent clip is left silent
    assert limiter.design(16000, peak=0.0)[0] == 1.0
    # ceiling 0 dBFS is full scale
    assert limiter.design(16000, ceiling_db=0, drive_db=0, peak=1.0)[:2] == (1.0, 1.0)
    # W from seconds: floor(s * rate + 0.5), at least 1, refused beyond the maximum with the longest time at that rate
    for rate, seconds, want in ((16000, 0.005, 80), (44100, 0.005, 221), (48000, 0.005, 240), (44100, 0.0050113, 221), (44100, 0.00501134, 221),
                                (16000, 0.0, 1), (48000, 1e-6, 1), (16000, 0.128, 2048), (48000, 2048 / 48000, 2048), (44100, 0.01, 441),
                                (44100, 1.5 / 44100, 2)):
        assert limiter.lookahead_samples(rate, seconds) == want == max(1, int(math.floor(seconds * rate + 0.5))), (rate, seconds)
    for rate, seconds, longest in ((16000, 0.13, "0.128000"), (44100, 0.05, "0.046440"), (48000, 0.043, "0.042667")):
        with pytest.raises(ValueError, match=f"longest look-ahead at this rate is {longest} seconds"):
            limiter.lookahead_samples(rate, seconds)
    bad = [(dict(ceiling_db=0.1), "ceiling_db must not be above 0"), (dict(drive_db=-0.5), "drive_db must not be negative"),
           (dict(ceiling_db=float("nan")), "ceiling_db must be a finite"), (dict(drive_db=float("inf")), "drive_db must be a finite"),
           (dict(lookahead_seconds=float("nan")), "lookahead_seconds must be a finite"), (dict(lookahead_seconds=-0.001), "lookahead_seconds must not be negative"),
           (dict(peak=float("nan")), "peak must be a finite"), (dict(peak=-1.0), "peak must not be negative"), (dict(ceiling_db="-1"), "ceiling_db must be a finite")]
    for kw, message in bad:
        with pytest.raises(ValueError, match=message):
            limiter.design(48000, **kw)
    for rate in (0, -48000, 48000.0, True):
        with pytest.raises(ValueError, match="rate must be a positive integer"):
            limiter.design(rate)


def test_limiter_apply_refusals():
    from gansynth_amd import limiter
    clip = torch.zeros(2, 64)
    for bad in (torch.zeros(3, 64), torch.zeros(0), torch.zeros(2, 64, dtype=torch.float64), np.zeros(8, np.float32), torch.zeros(1, 64)):
        with pytest.raises(ValueError, match="clip must be"):
            limiter.apply(bad, 48000, peak=1.0)
    for kw, message in ((dict(ceiling_db=1.0), "ceiling_db"), (dict(drive_db=-1.0), "drive_db"), (dict(lookahead_seconds=1.0), "longest look-ahead"),
                        (dict(peak=float("inf")), "peak must be a finite"), (dict(peak=torch.zeros(2)), "peak must be one number")):
        with pytest.raises(ValueError, match=message):
            limiter.apply(clip, 48000, **dict(dict(peak=1.0), **kw))


# --------------------------------------------------------------------------------------------------------------------- the ABI
def test_workspace_bytes_without_gpu():
    from gansynth_amd import _lib
    lib = _lib.load()
    for rows in (1, 2):
        for n, want in ((1, 16), (4096, 16), (4097, 16), (2 * 4096 + 1, 32), (48000 * 60, 704 * 8), (64000, 128), (1 << 40, (1 << 28) * 8)):
            assert lib.gs_limit_workspace_bytes(rows, n) == want == (-(-n // 4096) * 8 + 15) // 16 * 16, (rows, n)
    for rows, n in ((0, 100), (3, 100), (-1, 100), (1, 0), (2, -5), (1, (1 << 40) + 1)):
        assert lib.gs_limit_workspace_bytes(rows, n) == 0, (rows, n)


def test_gs_limit_refusals_without_gpu():
    """Every GS_ERR_ARG case of include/gansynth_hip.h, with its message; nothing is dereferenced or launched."""
    from gansynth_amd import _lib
    lib = _lib.load()
    X, OUT, PCM, PEAK, GAIN, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x400100, 0x500000
    good = dict(x=X, rows=2, n=1000, row_stride=1000, pre_gain=1.5, ceiling=0.9, lookahead=240, out=OUT, out_stride=1000, pcm=PCM, peak=PEAK,
                min_gain=GAIN, ws=WS, ws_bytes=16)
    order = ("x", "rows", "n", "row_stride", "pre_gain", "ceiling", "lookahead", "out", "out_stride", "pcm", "peak", "min_gain", "ws", "ws_bytes")
    bad = [(dict(rows=0), b"rows must be 1 or 2"), (dict(rows=3), b"rows must be 1 or 2"), (dict(n=0), b"n must be in"), (dict(n=-4), b"n must be in"),
           (dict(row_stride=999), b"row_stride 999 is below n 1000"), (dict(out_stride=999), b"out_stride 999 is below n 1000"),
           (dict(x=None), b"null pointer"), (dict(out=None), b"null pointer"),
           (dict(x=X + 2), b"misaligned"), (dict(out=OUT + 1), b"misaligned"), (dict(peak=PEAK + 2), b"misaligned"), (dict(min_gain=GAIN + 1), b"misaligned"),
           (dict(pcm=PCM + 1), b"misaligned"),
           (dict(ws=WS + 8), b"workspace too small or misaligned"), (dict(ws=None), b"workspace too small or misaligned"),
           (dict(ws_bytes=15), b"workspace too small or misaligned"), (dict(n=4097, row_stride=5000, out_stride=5000, ws_bytes=16), None),
           (dict(n=8193, row_stride=9000, out_stride=9000, ws_bytes=16), b"need 32"),
           (dict(pre_gain=0.0), b"pre_gain must be finite and positive"), (dict(pre_gain=-1.0), b"pre_gain must be finite and positive"),
           (dict(pre_gain=float("inf")), b"pre_gain must be finite and positive"), (dict(pre_gain=float("nan")), b"pre_gain must be finite and positive"),
           (dict(ceiling=0.0), b"ceiling must be in (0, 1]"), (dict(ceiling=1.5), b"ceiling must be in (0, 1]"), (dict(ceiling=-0.5), b"ceiling must be in (0, 1]"),
           (dict(ceiling=float("nan")), b"ceiling must be in (0, 1]"),
           (dict(lookahead=0), b"lookahead must be in [1, 2048]"), (dict(lookahead=2049), b"lookahead must be in [1, 2048]"), (dict(lookahead=-3), b"lookahead must be in"),
           (dict(out=X), b"overlap"), (dict(out=X + 4 * 1999), b"overlap"), (dict(out=X - 4 * 1999), b"overlap"), (dict(out=X + 4 * 500, rows=1), b"overlap")]
    for change, message in bad:
        if message is None:
            continue                                         # (that row needs a device: two tiles fit 16 bytes)
        a = dict(good, **change)
        assert lib.gs_limit(*[a[k] for k in order], None) == -1, change
        assert message in lib.gs_last_error(), (change, lib.gs_last_error())
    # x and out side by side are apart: only a null workspace is left to refuse
    for out in (X + 4 * 2000, X - 4 * 2000):
        a = dict(good, out=out, ws=None)
        assert lib.gs_limit(*[a[k] for k in order], None) == -1 and b"workspace" in lib.gs_last_error()


# ------------------------------------------------------------------------------------------------------------------ the driver
def test_driver_flags():
    import gan_synth_main as main
    args = main.parser.parse_args(["--synthesize", "score.mid"])
    assert args.limit is None and args.limit_drive == 6.0 and args.limit_lookahead == 0.005 and main.check_limit_args(args) is False
    assert main.check_limit_args(main.parser.parse_args([])) is False
    args = main.parser.parse_args(["--synthesize", "a.mid", "--limit", "-1", "--limit_drive", "9", "--limit_lookahead", "0.01"])
    assert (args.limit, args.limit_drive, args.limit_lookahead) == (-1.0, 9.0, 0.01) and main.check_limit_args(args) is True
    assert main.check_limit_args(main.parser.parse_args(["--synthesize", "a.mid", "--limit", "0", "--limit_drive", "0"])) is True
    bad = [(["--synthesize", "a.mid", "--limit_drive", "9"], "need --limit"), (["--synthesize", "a.mid", "--limit_lookahead", "0.01"], "need --limit"),
           (["--generate", "--limit", "-1"], "--synthesize only"), (["--synthesize", "a.mid", "--limit", "0.5"], "at most 0"),
           (["--synthesize", "a.mid", "--limit", "nan"], "at most 0"), (["--synthesize", "a.mid", "--limit=-inf"], "finite ceiling"),
           (["--synthesize", "a.mid", "--limit", "-1", "--limit_drive", "-2"], "--limit_drive must be"),
           (["--synthesize", "a.mid", "--limit", "-1", "--limit_drive", "inf"], "--limit_drive must be"),
           (["--synthesize", "a.mid", "--limit", "-1", "--limit_lookahead", "-0.001"], "--limit_lookahead must be"),
           (["--synthesize", "a.mid", "--limit", "-1", "--limit_lookahead", "nan"], "--limit_lookahead must be")]
    for argv, message in bad:
        with pytest.raises(SystemExit, match=message):
            main.check_limit_args(main.parser.parse_args(argv))
    with pytest.raises(SystemExit, match="--synthesize only"):     # main refuses before it touches a device
        main.main(main.parser.parse_args(["--generate", "--limit", "-1"]))
    with pytest.raises(SystemExit):
        main.parser.parse_args(["--limit", "loud"])
