"""GPU: gs_fftconv (gansynth_amd/csrc/fftconv.hip) against the float64 restatement of tests/reverb_ref.py, within 4 times the error of that
file's single-precision restatement of the same algorithm (RV.E_F32, measured without the kernel; tests/test_reverb_cpu.py holds the
restatement to it) -- at the sizes where the blocking can go wrong, for one and two rows, a shared and a per-row impulse, row strides that
put row 1 on and off 16 bytes, NaN in the stride padding.  The ONE peak, the quotient and the PCM bit for bit against RV.finish of the
kernel's own unnormalised fp32 clip (the finish is deterministic although the FFT is not bit-defined).  Delays (exact silence before the first
tap), wet = 0, determinism, the cache of prepared spectra, and the chain: GANSynth.synthesize -> reverb.apply and the driver's --reverb on
the reduced PGGAN of tests/test_notes_gpu.py.
Every figure is printed before it is asserted.  Where a case has no recorded entry in RV.E_F32 (delays, wet = 0, the chain) the bound is the
same rule evaluated in the test: 4 * e(convolve_f32) on that case's own input."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from tests import reverb_ref as RV

pytestmark = pytest.mark.gpu
B = RV.B
SENTINEL, PCM_SENTINEL, PAD = 12345.0, 77, 64


def _K():
    from gansynth_amd import kernels
    return kernels.get()


@functools.lru_cache(maxsize=None)
def _case(case):
    """The fixed draw of a case, its float64 reference and scale at (DRY, WET): computed once, never written to."""
    x, h = RV.draw(*case)
    ref, a = RV.convolve(x, h, RV.DRY, RV.WET), RV.scale(x, h, RV.DRY, RV.WET)
    for arr in (x, h, ref, a):
        arr.setflags(write=False)
    return x, h, ref, a


class _Raw:
    """gs_fftconv itself on one case: x inside a buffer whose stride padding is NaN, out and pcm inside buffers full of a sentinel, the
    spectrum prepared once.  `aligned`: row strides that are multiples of 4 floats on 16-byte bases.  Else strides of 1 mod 4 floats: row 0
    starts on 16 bytes and takes the 16-byte paths, row 1 does not and goes sample by sample; a single row is moved off by one float."""

    def __init__(self, case, aligned):
        from gansynth_amd import _lib
        n, m, rows, ir_rows = case
        x, h, _, _ = _case(case)
        self.K, self.lib = _K(), _K().lib
        self.rows, self.n, self.m, self.n_out = rows, n, m, n + m - 1
        self.design = _lib.GsFftConv()
        assert self.lib.gs_fftconv_design(n, m, rows, ir_rows, ctypes.byref(self.design)) == 0
        self.offset = 1 if (rows == 1 and not aligned) else 0
        self.row_stride = (n + 7) // 4 * 4 + (0 if aligned else 1)
        self.out_stride = (self.n_out + 7) // 4 * 4 + (0 if aligned else 1)
        ir_stride = m + 3
        xbuf = torch.full((self.offset + rows * self.row_stride,), float("nan"), device="cuda")
        self.x = xbuf[self.offset:].view(rows, self.row_stride)
        self.x[:, :n] = torch.tensor(x, device="cuda")
        hbuf = torch.full((ir_rows, ir_stride), float("nan"), device="cuda")
        hbuf[:, :m] = torch.tensor(h, device="cuda")
        self.spectrum = torch.empty(self.lib.gs_fftconv_spectrum_bytes(ctypes.byref(self.design)), dtype=torch.uint8, device="cuda")
        self.prepare(hbuf, ir_stride)
        self.ws = torch.empty(self.lib.gs_fftconv_workspace_bytes(ctypes.byref(self.design)), dtype=torch.uint8, device="cuda")

    def prepare(self, hbuf, ir_stride):
        from gansynth_amd import kernels
        code = self.lib.gs_fftconv_prepare(ctypes.byref(self.design), hbuf.data_ptr(), ir_stride, self.spectrum.data_ptr(), self.spectrum.numel(),
                                           kernels._stream())
        torch.cuda.synchronize()
        assert code == 0, self.lib.gs_last_error()

    def __call__(self, dry, wet, normalize=False, want_pcm=False, want_peak=True):
        """-> (out [rows, n_out] host fp32, pcm host int16 or None, peak float or None); nothing outside them was written."""
        from gansynth_amd import kernels
        rows, n_out, stride = self.rows, self.n_out, self.out_stride
        buf = torch.full((PAD + self.offset + rows * stride + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        out = buf[PAD + self.offset:PAD + self.offset + rows * stride].view(rows, stride)
        pbuf = torch.full((PAD + rows * n_out + PAD,), PCM_SENTINEL, dtype=torch.int16, device="cuda") if want_pcm else None
        peak = torch.full((1,), -1.0, device="cuda") if want_peak else None
        code = self.lib.gs_fftconv(ctypes.byref(self.design), self.spectrum.data_ptr(), self.spectrum.numel(), self.x.data_ptr(), self.row_stride,
                                   dry, wet, 1 if normalize else 0, out.data_ptr(), stride, None if pbuf is None else pbuf[PAD:].data_ptr(),
                                   None if peak is None else peak.data_ptr(), self.ws.data_ptr(), self.ws.numel(), kernels._stream())
        torch.cuda.synchronize()
        assert code == 0, self.lib.gs_last_error()
        assert (buf[:PAD + self.offset] == SENTINEL).all() and (buf[PAD + self.offset + rows * stride:] == SENTINEL).all()
        assert (out[:, n_out:] == SENTINEL).all()
        pcm = None
        if want_pcm:
            assert (pbuf[:PAD] == PCM_SENTINEL).all() and (pbuf[PAD + rows * n_out:] == PCM_SENTINEL).all()
            pcm = pbuf[PAD:PAD + rows * n_out].cpu().numpy()
            pcm = pcm if rows == 1 else pcm.reshape(n_out, rows)
        return out[:, :n_out].cpu().numpy(), pcm, (None if peak is None else float(peak))


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "off16"])
@pytest.mark.parametrize("case", RV.cases(), ids=lambda c: "n%d-m%d-rows%d-ir%d" % c)
def test_accuracy_tail_peak_and_finish(case, aligned):
    _, _, ref, a = _case(case)
    run = _Raw(case, aligned)
    y, none, peak = run(RV.DRY, RV.WET)
    assert none is None and y.dtype == np.float32 and y.shape == ref.shape and np.isfinite(y).all()      # (the NaN padding of x did not reach y)
    e = RV.error(y, ref, a)
    print(f"case {case} {'aligned' if aligned else 'off16'}: e = {e:.4g}, e(convolve_f32) = {RV.E_F32[case]:.4g}, bound {RV.tolerance(case):.4g}")
    assert e <= RV.tolerance(case)
    assert peak == float(np.abs(y).max())                                                               # exact
    # a quiet clip is left alone: PCM of y as it is
    want_peak, want_out, want_pcm = RV.finish(y, True)
    out, pcm, peak = run(RV.DRY, RV.WET, normalize=True, want_pcm=True)
    assert peak == float(want_peak) and np.array_equal(out, want_out) and np.array_equal(pcm, want_pcm)
    # four times as loud (an exact scaling): the peak is above 1 from the second size on, and the clip is divided by it
    loud, _, loud_peak = run(4 * RV.DRY, 4 * RV.WET)
    assert np.array_equal(loud, y * np.float32(4)) and loud_peak == 4 * float(np.abs(y).max())
    want_peak, want_out, want_pcm = RV.finish(loud, True)
    out, pcm, peak = run(4 * RV.DRY, 4 * RV.WET, normalize=True, want_pcm=True)
    print(f"  peak of the loud clip {float(want_peak):.4f}")
    assert case[0] == 5 or want_peak > 1
    assert peak == float(want_peak) and np.array_equal(out, want_out) and np.array_equal(pcm, want_pcm)
    out, pcm, peak = run(4 * RV.DRY, 4 * RV.WET, normalize=False, want_pcm=True, want_peak=False)          # clipped PCM of the clip as it is
    assert peak is None and np.array_equal(out, loud) and np.array_equal(pcm, RV.finish(loud, False)[2])


def _bound(x, h, dry, wet):
    """The rule of tests/reverb_ref.py evaluated on this input: -> (ref, A, 4 * e(convolve_f32))."""
    ref, a = RV.convolve(x, h, dry, wet), RV.scale(x, h, dry, wet)
    return ref, a, RV.FACTOR * RV.error(RV.convolve_f32(x, h, dry, wet), ref, a)


@pytest.mark.parametrize("d", RV.DELAYS)
def test_delays(d):
    """h = a unit impulse at d, dry = 0, wet = 1: x shifted by d within the bound, and EXACTLY 0 before d (both rows share the impulse)."""
    n = 2 * B + 5
    x = RV.draw(n, 1, 2, 1, seed=90 + d)[0]
    h = np.zeros(d + 1, dtype=np.float32)
    h[d] = 1
    ref, a, bound = _bound(x, h, 0.0, 1.0)
    assert np.array_equal(ref[:, d:].astype(np.float32), x) or np.abs(ref[:, d:] - x).max() < 1e-12
    out, none, peak = _K().fft_convolve(torch.from_numpy(x).cuda(), torch.from_numpy(h).cuda(), 0.0, 1.0, normalize=False)
    y = out.cpu().numpy()
    e = RV.error(y, ref, a)
    print(f"delay {d}: e = {e:.4g}, bound {bound:.4g}")
    assert y.shape == (2, n + d) and none is None and e <= bound
    assert (y[:, :d] == 0).all() and float(peak) == float(np.abs(y).max())


def test_wet_zero_is_the_dry_clip():
    n, m = 2 * B + 3, B + 7
    x, h = RV.draw(n, m, 2, 2, seed=5)
    dry = float(np.float32(0.6))
    ref, a, bound = _bound(x, h, dry, 0.0)
    out, _, _ = _K().fft_convolve(torch.from_numpy(x).cuda(), torch.from_numpy(h).cuda(), dry, 0.0, normalize=False)
    y = out.cpu().numpy()
    e = RV.error(y, ref, a)
    print(f"wet = 0: e = {e:.4g}, bound {bound:.4g}")
    assert e <= bound and (y[:, n:] == 0).all() and y.shape == (2, n + m - 1)


def test_determinism_and_the_spectrum_cache():
    K = _K()
    n, m = 5 * B + 17, 3 * B + 5
    x, h = RV.draw(n, m, 2, 2)
    xd, hd = torch.from_numpy(x).cuda(), torch.from_numpy(h).cuda()
    count = K.fftconv_prepares
    first = K.fft_convolve(xd, hd, RV.DRY, RV.WET, normalize=True, want_pcm=True)
    second = K.fft_convolve(xd, hd, RV.DRY, RV.WET, normalize=True, want_pcm=True)
    assert K.fftconv_prepares == count + 1                                                   # the same impulse tensor: ONE prepare
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    fresh = K.fft_convolve(xd, hd.clone(), RV.DRY, RV.WET, normalize=True, want_pcm=True)     # another tensor: a freshly prepared spectrum
    assert K.fftconv_prepares == count + 2 and all(torch.equal(a, b) for a, b in zip(first, fresh))
    mono = K.fft_convolve(xd[0], hd[0], RV.DRY, RV.WET, normalize=False)                      # a row of it, on its own
    assert mono[0].shape == (n + m - 1,) and torch.equal(mono[0], K.fft_convolve(xd, hd, RV.DRY, RV.WET, normalize=False)[0][0])
    hd[:, 0] += 1                                                                            # changed in place: prepared again
    prepares = K.fftconv_prepares
    changed = K.fft_convolve(xd, hd, RV.DRY, RV.WET, normalize=True, want_pcm=True)
    assert K.fftconv_prepares == prepares + 1 and not torch.equal(changed[0], first[0])
    # x as a view with rows off 16 bytes: taken as it is, the same numbers
    wide = torch.full((2, n + 1), float("nan"), device="cuda")
    wide[:, :n] = xd
    assert all(torch.equal(a, b) for a, b in zip(changed, K.fft_convolve(wide[:, :n], hd, RV.DRY, RV.WET, normalize=True, want_pcm=True)))


# ---------------------------------------------------------------------------------------------------------------- the chain
def _three_notes():
    return [dict(pitch=60, velocity=100, start=0.0, end=0.05, pan=-0.6), dict(pitch=67, velocity=90, start=0.02, end=0.08, pan=0.5),
            dict(pitch=48, velocity=127, start=0.04, end=0.1)]


def test_synthesize_then_reverb(gpu_store):
    from gansynth_amd import reverb
    from tests.test_notes_gpu import _model
    model = _model()
    data = json.dumps(_three_notes()).encode()
    kw = dict(batch_size=4, release_seconds=0.01, seed=2)
    clip = model.synthesize(data, normalize=False, sample_rate=48000, stereo=True, **kw)
    n = clip.shape[1]
    impulse = reverb.design_impulse(48000, 0.05, channels=2, seed=2, predelay=0.001).cuda()
    m = impulse.shape[1]
    assert clip.shape[0] == 2 and m == 48 + 2400
    mix = 0.25
    y, none, peak = reverb.apply(clip, impulse, mix=mix, normalize=False)
    host, h = clip.cpu().numpy(), impulse.cpu().numpy()
    ref, a, bound = _bound(host, h, float(np.float32(1.0 - mix)), float(np.float32(mix)))
    e = RV.error(y.cpu().numpy(), ref, a)
    print(f"chain: n = {n}, m = {m}, e = {e:.4g}, bound {bound:.4g}, peak {float(peak):.4f}")
    assert y.shape == (2, n + m - 1) and none is None and e <= bound
    out, pcm, peak = reverb.apply(clip, impulse, mix=mix, normalize=True, want_pcm=True)
    want_peak, want_out, want_pcm = RV.finish(y.cpu().numpy(), True)
    assert float(peak) == float(want_peak) and np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(pcm.cpu().numpy(), want_pcm)
    # a mono impulse on the stereo clip is shared by both channels; the mono clip of the same score takes it too
    shared = reverb.apply(clip, impulse[:1], mix=mix, normalize=False)[0]
    assert torch.equal(shared[0], y[0]) and not torch.equal(shared[1], y[1])
    mono = model.synthesize(data, normalize=False, sample_rate=48000, **kw)
    wet_mono, pcm_mono, _ = reverb.apply(mono, impulse[0], mix=mix, want_pcm=True)
    assert wet_mono.shape == (mono.shape[0] + m - 1,) and pcm_mono.shape == wet_mono.shape
    with pytest.raises(ValueError, match="a stereo impulse"):
        reverb.apply(mono, impulse)


def test_driver_reverb(gpu_store, tmp_path):
    """`gan_synth_main.py --synthesize score.json --reverb 0.3 --stereo --output_rate 48000` after building its model: n + m - 1 frames of
    two channels, the PCM of the direct call, no run of clipped samples -- and the same score without the flags is today's file.
    (Full scale is reached by the peak sample alone: 32767, or -32768 where that sample is negative, gs_summary_audio_s16's rule.)"""
    from scipy.io import wavfile
    import gan_synth_main as main
    from gansynth_amd import reverb
    from tests.test_notes_gpu import _model
    model = _model()
    (tmp_path / "score.json").write_text(json.dumps(_three_notes()))
    common = ["--synthesize", str(tmp_path / "score.json"), "--batch_size", "4", "--release_seconds", "0.01", "--model_dir", str(tmp_path / "no_model"),
              "--seed", "3"]
    args = main.parser.parse_args(common + ["--output", str(tmp_path / "wet.wav"), "--reverb", "0.3", "--stereo", "--output_rate", "48000"])
    lines = []
    info = main.synthesize_to_wav(model, args, range(24, 85), log=lines.append)
    rate, data = wavfile.read(str(tmp_path / "wet.wav"))
    clip = model.synthesize(str(tmp_path / "score.json"), normalize=False, sample_rate=48000, stereo=True, batch_size=4, release_seconds=0.01, seed=3)
    n, m = clip.shape[1], 14400
    assert rate == 48000 and data.dtype == np.int16 and data.shape == (n + m - 1, 2)
    assert info["output_samples"] == n + m - 1 and info["reverb_tail"] == m - 1 and info["sample_rate"] == 48000 and info["channels"] == 2
    impulse = reverb.design_impulse(48000, 0.3, channels=2, seed=3)
    out, pcm, peak = reverb.apply(clip, impulse.cuda(), mix=0.25, normalize=True, want_pcm=True)
    assert np.array_equal(data, pcm.cpu().numpy()) and info["peak"] == float(peak) and np.abs(data[n:]).max() > 0        # the tail sounds
    wide = np.abs(data.astype(np.int32))
    full = wide >= 32767
    print(f"driver: peak {float(peak):.4f}, largest |pcm| {wide.max()}, samples at full scale {full.sum()}")
    assert float(out.abs().max()) <= 1.0 and data.max() <= 32767 and wide.max() <= 32768
    assert not (full[1:] & full[:-1]).any()                                              # no two successive frames of a channel at full scale
    assert f"reverb tail of {m - 1} samples" in lines[-1] and "peak" in lines[-1]
    # without the flags: the file of a plain synthesize call
    args = main.parser.parse_args(common + ["--output", str(tmp_path / "dry.wav"), "--stereo", "--output_rate", "48000"])
    info = main.synthesize_to_wav(model, args, range(24, 85), log=lines.append)
    rate, dry = wavfile.read(str(tmp_path / "dry.wav"))
    _, want = model.synthesize(str(tmp_path / "score.json"), want_pcm=True, sample_rate=48000, stereo=True, batch_size=4, release_seconds=0.01, seed=3)
    assert rate == 48000 and np.array_equal(dry, want.cpu().numpy()) and dry.shape == (n, 2) and "reverb_tail" not in info
    assert "reverb tail" not in lines[-1]
