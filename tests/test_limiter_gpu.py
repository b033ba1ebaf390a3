"""GPU: gs_limit (gansynth_amd/csrc/limiter.hip) against the float64 restatement of tests/limiter_ref.py, within 4 times the error of that
file's single-precision restatement on the same case (LR.FACTOR: the project's margin, not tuned to the kernel) -- at the lengths
{1, 2, W, W + 1, T - 1, T, T + 1, 3T + 5} and the look-aheads {1, 63, 64, 65, 240, 2048} (and 256, 257, 1024, 1025, where the entry point
changes its kernel, at three lengths), one and two rows, row strides that put the rows on and
off 16 bytes, with spikes at both ends, on each side of every tile seam, W and W + 1 before a seam, a plateau across a seam and a spike in one
channel alone (LR.draw).  A short clip is drawn LR.draws(n) times and the maxima run over all its draws (the reason is written there).
The exact properties -- |out| <= c, out == fl(d * x) where quiet, the PCM, the peak, the least gain, determinism, untouched padding, a NaN
sample -- hold bit for bit.  Then the Python layer and the driver's --limit on the reduced PGGAN of tests/test_notes_gpu.py.
Every figure is printed before it is asserted."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import limiter_ref as LR

pytestmark = pytest.mark.gpu
C, D, T = LR.C, LR.D, LR.T
SENTINEL, PCM_SENTINEL, PAD = 12345.0, 77, 64


def _K():
    from gansynth_amd import kernels
    return kernels.get()


@functools.lru_cache(maxsize=None)
def _case(n, rows, W, k):
    """Draw k of a case with its references: computed once, never written to."""
    x = LR.draw(n, rows, W, k=k)
    y = LR.pre(x, D)
    ref, f32 = LR.limit_f64(y, C, W), LR.limit_f32(y, C, W)
    for arr in (x, y) + tuple(ref) + tuple(f32):
        arr.setflags(write=False)
    return x, y, ref, f32


def _run(x, d, c, W, aligned, want_pcm=True, want_stats=True):
    """gs_limit itself on x [rows, n]: x inside a buffer whose stride padding is NaN, out and pcm inside buffers full of a sentinel.
    `aligned`: row strides that are multiples of 4 floats on 16-byte bases.  Else strides of 1 mod 4 floats -- row 1 is off 16 bytes -- and a
    single row moved off by one float: the sample-by-sample path.  -> (out [rows, n], pcm, peak, min_gain) on the host; nothing outside
    them was written."""
    from gansynth_amd import kernels
    lib = _K().lib
    rows, n = x.shape
    offset = 1 if (rows == 1 and not aligned) else 0
    stride = (n + 7) // 4 * 4 + (0 if aligned else 1)
    xbuf = torch.full((offset + rows * stride,), float("nan"), device="cuda")
    xv = xbuf[offset:].view(rows, stride)
    xv[:, :n] = torch.tensor(x, device="cuda")
    buf = torch.full((PAD + offset + rows * stride + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[PAD + offset:PAD + offset + rows * stride].view(rows, stride)
    pbuf = torch.full((PAD + rows * n + PAD,), PCM_SENTINEL, dtype=torch.int16, device="cuda") if want_pcm else None
    peak = torch.full((1,), -1.0, device="cuda") if want_stats else None
    gain = torch.full((1,), -1.0, device="cuda") if want_stats else None
    ws = torch.empty(max(int(lib.gs_limit_workspace_bytes(rows, n)), 16), dtype=torch.uint8, device="cuda")
    assert (xv.data_ptr() % 16 == 0) == (offset == 0) and (out.data_ptr() % 16 == 0) == (offset == 0)
    code = lib.gs_limit(xv.data_ptr(), rows, n, stride, float(d), float(c), int(W), out.data_ptr(), stride,
                        None if pbuf is None else pbuf[PAD:].data_ptr(), None if peak is None else peak.data_ptr(),
                        None if gain is None else gain.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream())
    torch.cuda.synchronize()
    assert code == 0, lib.gs_last_error()
    assert (buf[:PAD + offset] == SENTINEL).all() and (buf[PAD + offset + rows * stride:] == SENTINEL).all()
    assert (out[:, n:] == SENTINEL).all()                                    # between n and out_stride: untouched
    pcm = None
    if want_pcm:
        assert (pbuf[:PAD] == PCM_SENTINEL).all() and (pbuf[PAD + rows * n:] == PCM_SENTINEL).all()
        pcm = pbuf[PAD:PAD + rows * n].cpu().numpy()
        pcm = pcm if rows == 1 else pcm.reshape(n, rows)
    return out[:, :n].cpu().numpy(), pcm, (None if peak is None else float(peak)), (None if gain is None else float(gain))


def _exact(out, pcm, peak, gain, y, c, W):
    """The properties that hold bit for bit, on what one call returned."""
    c = np.float32(c)
    finite = ~np.isnan(y)
    assert out.dtype == np.float32 and out.shape == y.shape and np.array_equal(np.isnan(out), ~finite)
    assert (np.abs(out[finite]) <= c).all()
    quiet = LR.quiet(y, c, W)[None, :] & finite
    assert np.array_equal(out[quiet].view(np.uint32), y[quiet].view(np.uint32))
    assert np.array_equal(pcm, LR.pcm(out))
    assert np.float32(peak) == LR.peak(out)
    # the least gain: no sample was scaled by less, and (where no spike was clamped to the ceiling itself) one was scaled by exactly it
    assert 0 < gain <= 1
    least = np.abs((np.float32(gain) * y).astype(np.float32))
    free = finite & (np.abs(out) < c)
    assert (least[free] <= np.abs(out)[free]).all()
    assert gain == 1 or (np.minimum(least, c)[finite] == np.abs(out)[finite]).any()


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "off16"])
@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("W,n", [(W, n) for W in LR.LOOKAHEADS for n in LR.lengths(W)] + [(W, n) for W in LR.EDGE_LOOKAHEADS for n in (W, T + 1, 3 * T + 5)],
                         ids=lambda v: str(v))
def test_against_the_restatement(W, n, rows, aligned):
    e_out = e_g = b_out = b_g = 0.0
    for k in range(LR.draws(n)):
        x, y, ref, f32 = _case(n, rows, W, k)
        out, pcm, peak, gain = _run(x, D, C, W, aligned)
        _exact(out, pcm, peak, gain, y, C, W)
        e_out, b_out = max(e_out, LR.out_error(out, ref)), max(b_out, LR.out_error(f32.out, ref))
        e_g, b_g = max(e_g, LR.gain_error(out, ref, C, gain)), max(b_g, LR.gain_error(f32.out, ref, C, f32.g.min()))
        if k == 0:                                                            # two calls: byte-identical
            again = _run(x, D, C, W, aligned)
            assert np.array_equal(again[0].view(np.uint32), out.view(np.uint32)) and np.array_equal(again[1], pcm) and again[2:] == (peak, gain)
    print(f"W {W} n {n} rows {rows} {'aligned' if aligned else 'off16'} ({LR.draws(n)} draws): out {e_out:.3g} against limit_f32's {b_out:.3g} "
          f"(ratio {e_out / b_out if b_out else 0:.3f}), g {e_g:.3g} against {b_g:.3g} (ratio {e_g / b_g if b_g else 0:.3f})")
    assert e_out <= LR.FACTOR * b_out and e_g <= LR.FACTOR * b_g


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "off16"])
@pytest.mark.parametrize("rows", [1, 2])
def test_a_clip_below_the_ceiling_is_only_scaled(rows, aligned):
    n = 3 * T + 5
    x = (LR.draw(n, rows, 64, seed=21) * np.float32(0.3)).astype(np.float32)
    y = LR.pre(x, D)
    assert np.abs(y).max() <= C
    for W in (1, 240, 2048):
        out, pcm, peak, gain = _run(x, D, C, W, aligned)
        assert np.array_equal(out.view(np.uint32), y.view(np.uint32)) and gain == 1.0 and np.float32(peak) == np.abs(y).max()
        assert np.array_equal(pcm, LR.pcm(y))
    only, none, no_peak, no_gain = _run(x, D, C, 240, aligned, want_pcm=False, want_stats=False)       # the optional outputs left out
    assert none is None and no_peak is None and no_gain is None and np.array_equal(only, y)


@pytest.mark.parametrize("where", [0, T - 1, T, 2 * T + 3])
def test_a_nan_sample_stays_alone(where):
    n, W = 2 * T + 9, 240
    x = LR.draw(n, 2, W, seed=30).copy()
    zeroed = x.copy()
    zeroed[1, where] = 0
    x[1, where] = np.nan
    for aligned in (True, False):
        out, pcm, peak, gain = _run(x, D, C, W, aligned)
        want, want_pcm, want_peak, want_gain = _run(zeroed, D, C, W, aligned)
        _exact(out, pcm, peak, gain, LR.pre(x, D), C, W)
        assert np.isnan(out[1, where]) and pcm[where, 1] == 0 and (peak, gain) == (want_peak, want_gain)
        keep = np.ones(out.shape, dtype=bool)
        keep[1, where] = False
        assert np.array_equal(out[keep], want[keep]) and np.array_equal(pcm.reshape(-1, 2)[keep.T], want_pcm.reshape(-1, 2)[keep.T])
        ref = LR.limit_f64(LR.pre(zeroed, D), C, W)
        f32 = LR.limit_f32(LR.pre(zeroed, D), C, W)
        assert LR.out_error(want, ref) <= LR.FACTOR * LR.out_error(f32.out, ref)


def test_the_python_layer():
    from gansynth_amd import kernels, limiter
    K = _K()
    W = 64
    x, y, ref, f32 = _case(T + 1, 2, W, 0)
    xd = torch.tensor(x, device="cuda")
    out, pcm, peak, gain = K.limit(xd, float(D), float(C), W, want_pcm=True)
    raw = _run(x, D, C, W, True)
    assert out.shape == (2, T + 1) and pcm.shape == (T + 1, 2) and peak.shape == (1,) and gain.shape == (1,)
    assert np.array_equal(out.cpu().numpy(), raw[0]) and np.array_equal(pcm.cpu().numpy(), raw[1]) and (float(peak), float(gain)) == raw[2:]
    assert out.data_ptr() != xd.data_ptr() and np.array_equal(xd.cpu().numpy(), x)                     # x is left as it was
    mono = kernels.limit(xd[0], float(D), float(C), W)                                              # one row of it: its own gain
    assert mono[0].shape == (T + 1,) and mono[1] is None
    assert np.array_equal(mono[0].cpu().numpy(), _run(x[:1], D, C, W, True)[0][0])
    wide = torch.full((2, T + 2), float("nan"), device="cuda")                                      # a view with rows off 16 bytes: taken as it is
    wide[:, :T + 1] = xd
    assert torch.equal(K.limit(wide[:, :T + 1], float(D), float(C), W)[0], out)
    with pytest.raises(ValueError, match="must be on the HIP device"):
        K.limit(xd.cpu(), 1.0, 0.9, 8)
    # limiter.apply: the design's numbers, the peak taken here or handed over
    clip = xd * 3
    got = limiter.apply(clip, 48000, ceiling_db=-1.0, drive_db=6.0, lookahead_seconds=0.005, want_pcm=True)
    pre_gain, c, w = limiter.design(48000, -1.0, 6.0, 0.005, float(clip.abs().max()))
    want = K.limit(clip, pre_gain, c, w, want_pcm=True)
    assert w == 240 and all(torch.equal(a, b) for a, b in zip(got, want))
    handed = limiter.apply(clip, 48000, peak=clip.abs().max().reshape(1), want_pcm=True)
    assert all(torch.equal(a, b) for a, b in zip(handed, want))
    assert float(got[2]) <= np.float32(c) and float(got[3]) < 1
    flat = limiter.apply(clip, 48000, drive_db=0.0)                                                 # drive 0: the peak on the ceiling, the gain 1
    assert float(flat[3]) == 1.0 and abs(float(flat[2]) - c) <= 2.0 ** -22


# ---------------------------------------------------------------------------------------------------------------- the driver
def _four_notes():
    return [dict(pitch=60, velocity=100, start=0.0, end=0.05, pan=-0.6), dict(pitch=67, velocity=90, start=0.02, end=0.08, pan=0.5),
            dict(pitch=48, velocity=127, start=0.04, end=0.1), dict(pitch=72, velocity=110, start=0.05, end=0.11, pan=0.2)]


def test_driver_limit(gpu_store, tmp_path):
    """`gan_synth_main.py --synthesize score.json --stereo --output_rate 48000 --reverb 0.3 --limit -1 --limit_drive 9` after building its
    model: no sample of the file beyond round(c * 32768), louder (RMS) than the same render without --limit; --limit_drive 0 is the peak
    normalisation to the ceiling within 1 LSB; and without the flag the file is the one of tests/test_reverb_gpu.py's chain."""
    from scipy.io import wavfile
    import gan_synth_main as main
    from gansynth_amd import reverb
    from tests.test_notes_gpu import _model
    model = _model()
    (tmp_path / "score.json").write_text(json.dumps(_four_notes()))
    common = ["--synthesize", str(tmp_path / "score.json"), "--batch_size", "4", "--release_seconds", "0.01", "--model_dir", str(tmp_path / "no_model"),
              "--seed", "3", "--stereo", "--output_rate", "48000", "--reverb", "0.3"]
    c = 10.0 ** (-1.0 / 20)
    lines = []

    def render(name, extra):
        args = main.parser.parse_args(common + ["--output", str(tmp_path / name)] + extra)
        info = main.synthesize_to_wav(model, args, range(24, 85), log=lines.append)
        rate, data = wavfile.read(str(tmp_path / name))
        assert rate == 48000 and data.dtype == np.int16 and data.ndim == 2 and data.shape[1] == 2
        return info, data.astype(np.int64)

    info, limited = render("limited.wav", ["--limit", "-1", "--limit_drive", "9"])
    plain_info, plain = render("plain.wav", [])
    assert limited.shape == plain.shape and "limit_min_gain" not in plain_info and "limited to" not in lines[-1]
    rms = [float(np.sqrt((d.astype(np.float64) ** 2).mean())) for d in (limited, plain)]
    print(f"driver: largest |pcm| {np.abs(limited).max()} against round(c * 32768) = {round(c * 32768)}, RMS {rms[0]:.1f} against {rms[1]:.1f} without "
          f"--limit, least gain {info['limit_min_gain']:.4f}, peak {info['limit_peak']:.6f}")
    assert np.abs(limited).max() <= round(c * 32768) and info["limit_peak"] <= np.float32(c)
    assert rms[0] > rms[1] and info["limit_min_gain"] < 1
    assert info["limit_ceiling_db"] == -1.0 and info["limit_drive_db"] == 9.0
    written = [line for line in lines if "written to" in line]
    assert "limited to -1 dBFS with 9 dB of drive, deepest gain reduction" in written[0] and "reverb tail" in written[0]
    # drive 0: peak normalisation to the ceiling
    info, flat = render("flat.wav", ["--limit", "-1", "--limit_drive", "0"])
    clip = model.synthesize(str(tmp_path / "score.json"), normalize=False, sample_rate=48000, stereo=True, batch_size=4, release_seconds=0.01, seed=3)
    impulse = reverb.design_impulse(48000, 0.3, channels=2, seed=3)
    y, _, peak = reverb.apply(clip, impulse.cuda(), mix=0.25, normalize=False)
    want = LR.pcm(y.cpu().numpy().astype(np.float64) * c / float(peak)).astype(np.int64)
    print(f"drive 0: largest difference to the normalised clip {np.abs(flat - want).max()} LSB, least gain {info['limit_min_gain']}")
    assert flat.shape == want.shape and np.abs(flat - want).max() <= 1 and info["limit_min_gain"] == 1.0
    # without the flag: the file of the chain as it was (reverb.apply normalising and quantising)
    _, pcm, _ = reverb.apply(clip, impulse.cuda(), mix=0.25, normalize=True, want_pcm=True)
    assert np.array_equal(plain, pcm.cpu().numpy().astype(np.int64))
