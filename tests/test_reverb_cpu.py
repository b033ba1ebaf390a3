"""CPU: the reverb (DESIGN.md "Reverb") without a device -- the host queries of gs_fftconv against hand arithmetic, every refusal of the entry
points (no launch, no pointer dereferenced), the refusals of kernels.fft_convolve and reverb.apply by argument name, reverb.design_impulse
against the restatement of tests/reverb_ref.py, reverb.read_impulse on files written here, the fp32 restatement inside a quarter of the
GPU test's tolerance on every GPU case, and the driver's four flags."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import reverb_ref as RV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = RV.B
HEADER = (2048 + 1024 + 8) * 8 + 16      # stage twiddles, pack twiddles (B/2 + 1 padded to B/2 + 8), lead[2] padded to 16 bytes
# (n, m) -> (P, J, XB) by hand: P = ceil(m / B), J = ceil((n + m - 1) / B), XB = min(J, floor((n - 1) / B) + 2)
COUNTS = {(5, 1): (1, 1, 1), (B - 1, 2): (1, 1, 1), (B, B): (1, 2, 2), (B + 1, B + 1): (2, 3, 3), (5 * B + 17, 3 * B + 5): (4, 9, 7),
          (2 * B + 3, 6 * B - 1): (6, 9, 4), (2880000, 96000): (47, 1454, 1408), (64000, 16000): (8, 40, 33)}


def _design(n, m, rows=1, ir_rows=1):
    from gansynth_amd import _lib
    lib = _lib.load()
    d = _lib.GsFftConv()
    assert lib.gs_fftconv_design(n, m, rows, ir_rows, ctypes.byref(d)) == 0, lib.gs_last_error()
    return _lib, lib, d


def test_host_queries_against_hand_arithmetic():
    assert B == 2048 and HEADER == 24656 and sorted(RV.SIZES) == sorted(k for k in COUNTS if k[0] < 60000)
    for (n, m), (parts, blocks, x_blocks) in COUNTS.items():
        for rows, ir_rows in RV.ROWS:
            _, lib, d = _design(n, m, rows, ir_rows)
            assert (d.n, d.m, d.rows, d.ir_rows, d.block) == (n, m, rows, ir_rows, B)
            assert (d.partitions, d.blocks, d.x_blocks) == (parts, blocks, x_blocks) == (-(-m // B), -(-(n + m - 1) // B), min(blocks, (n - 1) // B + 2))
            assert lib.gs_fftconv_out_len(ctypes.byref(d)) == n + m - 1
            assert lib.gs_fftconv_spectrum_bytes(ctypes.byref(d)) == HEADER + ir_rows * parts * B * 8
            assert lib.gs_fftconv_workspace_bytes(ctypes.byref(d)) == rows * x_blocks * B * 8 + rows * blocks * 4
    _, lib, d = _design(1, 1)
    assert (d.partitions, d.blocks, d.x_blocks) == (1, 1, 1) and lib.gs_fftconv_out_len(ctypes.byref(d)) == 1
    _, lib, d = _design(1 << 40, 1 << 20, 2, 2)
    assert (d.partitions, d.blocks, d.x_blocks) == (512, (1 << 29) + 512, (1 << 29) + 1)


def test_descriptor_mirror_and_constants():
    from gansynth_amd import _lib, reverb
    hdr = open(os.path.join(ROOT, "include", "gansynth_hip.h")).read()
    assert int(re.search(r"#define GS_FFTCONV_BLOCK (\d+)", hdr).group(1)) == _lib.FFTCONV_BLOCK == B
    assert re.search(r"#define GS_FFTCONV_MAX_TAPS \(1 << (\d+)\)", hdr).group(1) == "20" and _lib.FFTCONV_MAX_TAPS == 1 << 20 == reverb.MAX_TAPS
    assert _lib.FFTCONV_HEADER_BYTES == HEADER
    assert ctypes.sizeof(_lib.GsFftConv) == 40
    assert [(n, getattr(_lib.GsFftConv, n).offset) for n, _ in _lib.GsFftConv._fields_] == \
        [("n", 0), ("m", 8), ("rows", 16), ("ir_rows", 20), ("block", 24), ("partitions", 28), ("blocks", 32), ("x_blocks", 36)]


def test_refusals_without_gpu():
    from gansynth_amd import _lib
    lib = _lib.load()
    d = _lib.GsFftConv()
    for n, m, rows, ir_rows, message in ((0, 5, 1, 1, b"n must"), (-3, 5, 1, 1, b"n must"), ((1 << 40) + 1, 5, 1, 1, b"n must"), (5, 0, 1, 1, b"m must"),
                                         (5, -1, 1, 1, b"m must"), (5, (1 << 20) + 1, 1, 1, b"taps"), (5, 5, 0, 1, b"rows must"), (5, 5, -2, 1, b"rows must"),
                                         (5, 5, 3, 1, b"rows must"), (5, 5, 2, 0, b"ir_rows"), (5, 5, 2, 3, b"ir_rows"), (5, 5, 1, 2, b"ir_rows")):
        assert lib.gs_fftconv_design(n, m, rows, ir_rows, ctypes.byref(d)) == -1, (n, m, rows, ir_rows)      # GS_ERR_ARG
        assert message in lib.gs_last_error(), (n, m, rows, ir_rows, lib.gs_last_error())
    assert lib.gs_fftconv_design(5, 5, 1, 1, None) == -1 and b"null" in lib.gs_last_error()

    n, m = 5 * B + 17, 3 * B + 5
    _, lib, d = _design(n, m, 2, 2)
    n_out = n + m - 1
    spectrum_bytes, ws_bytes = lib.gs_fftconv_spectrum_bytes(ctypes.byref(d)), lib.gs_fftconv_workspace_bytes(ctypes.byref(d))
    P = 0x10000   # (never dereferenced: the argument checks come first and nothing is launched)
    good = dict(c=ctypes.byref(d), spectrum=P, spectrum_bytes=spectrum_bytes, x=P, row_stride=n + 3, dry=0.75, wet=0.25, normalize=1, out=P,
                out_stride=n_out + 1, pcm=None, peak=None, ws=P, ws_bytes=ws_bytes, stream=None)
    order = ["c", "spectrum", "spectrum_bytes", "x", "row_stride", "dry", "wet", "normalize", "out", "out_stride", "pcm", "peak", "ws", "ws_bytes", "stream"]
    bad = [("row_stride", n - 1, b"row_stride"), ("out_stride", n_out - 1, b"out_stride"), ("x", None, b"null"), ("out", None, b"null"),
           ("spectrum", None, b"null"), ("x", P + 2, b"misaligned"), ("out", P + 1, b"misaligned"), ("peak", P + 2, b"misaligned"),
           ("pcm", P + 1, b"misaligned"), ("spectrum", P + 8, b"misaligned"), ("spectrum_bytes", spectrum_bytes - 1, b"spectrum buffer too small"),
           ("ws_bytes", ws_bytes - 1, b"workspace"), ("ws", None, b"workspace"), ("ws", P + 8, b"workspace"), ("c", None, b"descriptor")]
    for field, value, message in bad:
        args = dict(good, **{field: value})
        assert lib.gs_fftconv(*[args[k] for k in order]) == -1, (field, value)
        assert message in lib.gs_last_error(), (field, value, lib.gs_last_error())
    pgood = dict(c=ctypes.byref(d), ir=P, ir_stride=m, spectrum=P, spectrum_bytes=spectrum_bytes, stream=None)
    porder = ["c", "ir", "ir_stride", "spectrum", "spectrum_bytes", "stream"]
    for field, value, message in (("ir", None, b"null"), ("spectrum", None, b"null"), ("ir", P + 2, b"misaligned"), ("spectrum", P + 4, b"misaligned"),
                                  ("ir_stride", m - 1, b"ir_stride"), ("spectrum_bytes", spectrum_bytes - 1, b"spectrum buffer too small"),
                                  ("c", None, b"descriptor")):
        args = dict(pgood, **{field: value})
        assert lib.gs_fftconv_prepare(*[args[k] for k in porder]) == -1, (field, value)
        assert message in lib.gs_last_error(), (field, value, lib.gs_last_error())
    # a descriptor that does not follow from its n and m, one field at a time -- and values no design exists for
    for field, value, message in (("block", 1024, b"does not follow"), ("block", 4096, b"does not follow"), ("partitions", d.partitions + 1, b"does not follow"),
                                  ("partitions", d.partitions - 1, b"does not follow"), ("blocks", d.blocks + 1, b"does not follow"),
                                  ("blocks", d.blocks - 1, b"does not follow"), ("x_blocks", d.x_blocks + 1, b"does not follow"), ("x_blocks", 0, b"does not follow"),
                                  ("n", n + B, b"does not follow"), ("m", m + B, b"does not follow"), ("n", 0, b"n must"), ("m", (1 << 20) + 1, b"taps"),
                                  ("rows", 3, b"rows must"), ("ir_rows", 3, b"ir_rows")):
        wrong = _lib.GsFftConv(d.n, d.m, d.rows, d.ir_rows, d.block, d.partitions, d.blocks, d.x_blocks)
        setattr(wrong, field, value)
        assert lib.gs_fftconv(*[dict(good, c=ctypes.byref(wrong))[k] for k in order]) == -1, (field, value)
        assert message in lib.gs_last_error(), (field, value, lib.gs_last_error())
        assert lib.gs_fftconv_prepare(*[dict(pgood, c=ctypes.byref(wrong))[k] for k in porder]) == -1, (field, value)
        assert lib.gs_fftconv_out_len(ctypes.byref(wrong)) == -1
        assert lib.gs_fftconv_spectrum_bytes(ctypes.byref(wrong)) == 0 and lib.gs_fftconv_workspace_bytes(ctypes.byref(wrong)) == 0
    assert lib.gs_fftconv_out_len(None) == -1 and lib.gs_fftconv_spectrum_bytes(None) == 0 and lib.gs_fftconv_workspace_bytes(None) == 0


def test_python_refusals_name_the_argument():
    from gansynth_amd import kernels, reverb
    x, h = torch.zeros(2, 100), torch.zeros(2, 10)
    for args, name in (((torch.zeros(2, 3, 4), h, 1.0, 0.5), "x"), ((x.double(), h, 1.0, 0.5), "x"), ((torch.zeros(0), h[0], 1.0, 0.5), "x"),
                       ((torch.zeros(3, 100), h[0], 1.0, 0.5), "x"), ((x, torch.zeros(2, 2, 2), 1.0, 0.5), "impulse"), ((x, h.half(), 1.0, 0.5), "impulse"),
                       ((x, torch.zeros(1, 0), 1.0, 0.5), "impulse"), ((x, torch.zeros(3, 10), 1.0, 0.5), "impulse"), ((x[0], h, 1.0, 0.5), "impulse"),
                       ((x, [1.0, 2.0], 1.0, 0.5), "impulse"), ((x, h, float("nan"), 0.5), "dry"), ((x, h, 1.0, "much"), "wet"),
                       ((x, h, 1.0, float("inf")), "wet")):
        with pytest.raises(ValueError, match=f"fft_convolve: {name} "):
            kernels.fft_convolve(*args)
    assert kernels.fft_convolve_shapes(x, h, 1.0, 0.5) == (2, 100, 2, 10) and kernels.fft_convolve_shapes(x, h[0], 1, 0) == (2, 100, 1, 10)
    assert kernels.fft_convolve_shapes(x[0], h[:1], 0.5, 0.5) == (1, 100, 1, 10)
    for args, kw, name in (((x, h), dict(mix=1.5), "mix"), ((x, h), dict(mix=-0.1), "mix"), ((x, h), dict(mix=None), "mix"), ((torch.zeros(3, 100), h), {}, "clip"),
                           ((x.double(), h), {}, "clip"), ((torch.zeros(2, 0), h), {}, "clip"), ((np.zeros(5, dtype=np.float32), h), {}, "clip"),
                           ((x, torch.zeros(3, 10)), {}, "impulse"), ((x, h.double()), {}, "impulse"), ((x, torch.zeros(2, 2, 2)), {}, "impulse"),
                           ((x[0], h), {}, "a stereo impulse")):
        with pytest.raises(ValueError, match=f"reverb.apply: {name}"):
            reverb.apply(*args, **kw)


def test_design_impulse_is_the_restatement():
    from gansynth_amd import reverb
    numpy_state, torch_state = np.random.get_state(), torch.get_rng_state()
    for rate, rt60, channels, seed, predelay in ((16000, 0.25, 1, 0, 0.0), (16000, 0.25, 2, 0, 0.0), (48000, 0.1, 2, 7, 0.0105), (48000, 0.0333, 1, 3, 0.002)):
        h = reverb.design_impulse(rate, rt60, channels=channels, seed=seed, predelay=predelay)
        pre, length = int(np.floor(predelay * rate + 0.5)), int(np.ceil(rt60 * rate))
        assert isinstance(h, torch.Tensor) and h.dtype == torch.float32 and not h.is_cuda and tuple(h.shape) == (channels, pre + length)
        got = h.numpy()
        assert np.array_equal(got, RV.design_impulse(rate, rt60, channels, seed, predelay))                      # element for element
        assert (got[:, :pre] == 0).all() and (got[:, pre] != 0).all()
        norms = np.sqrt((got.astype(np.float64) ** 2).sum(axis=1))
        assert abs(norms.max() - 1) <= 2.0 ** -23 and (norms > 0.5).all()
        # the envelope's last value: the draw divided out again, 10 ** (-3 (L - 1) / (rt60 rate)) within fp32 rounding
        g = np.random.Generator(np.random.PCG64(seed)).standard_normal((channels, length))
        top = np.sqrt(((g * 10.0 ** (-3.0 * np.arange(length) / (rt60 * rate))) ** 2).sum(axis=1)).max()
        last = got[:, -1].astype(np.float64) * top / g[:, -1]
        assert np.allclose(last, 10.0 ** (-3.0 * (length - 1) / (rt60 * rate)), rtol=2.0 ** -22, atol=0)
        if channels == 2:
            assert not np.array_equal(got[0], got[1])
        assert torch.equal(h, reverb.design_impulse(rate, rt60, channels=channels, seed=seed, predelay=predelay))   # two calls
    assert not torch.equal(reverb.design_impulse(16000, 0.1, seed=1), reverb.design_impulse(16000, 0.1, seed=2))
    assert tuple(reverb.design_impulse(16000, 0.1, predelay=0.00103).shape) == (1, 16 + 1600)     # floor(16.48 + 0.5): rounded to the nearest sample
    assert tuple(reverb.design_impulse(16000, 0.1, predelay=0.00097).shape) == (1, 16 + 1600)     # floor(15.52 + 0.5)
    assert tuple(reverb.design_impulse(16000, 0.10001).shape) == (1, 1601)                        # ceil(1600.16)
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(numpy_state, np.random.get_state()))
    assert torch.equal(torch_state, torch.get_rng_state())
    for kw, name in ((dict(rate=0, rt60=1.0), "rate"), (dict(rate=-16000, rt60=1.0), "rate"), (dict(rate=16000.5, rt60=1.0), "rate"),
                     (dict(rate=16000, rt60=0.0), "rt60"), (dict(rate=16000, rt60=-1.0), "rt60"), (dict(rate=16000, rt60=float("nan")), "rt60"),
                     (dict(rate=16000, rt60=1.0, predelay=-0.001), "predelay"), (dict(rate=16000, rt60=1.0, channels=3), "channels"),
                     (dict(rate=48000, rt60=22.0), "taps"), (dict(rate=48000, rt60=21.0, predelay=1.0), "taps")):
        with pytest.raises(ValueError, match=name):
            reverb.design_impulse(**kw)
    assert reverb.design_impulse(48000, 21.0).shape[1] == 1008000 <= reverb.MAX_TAPS


def test_read_impulse(tmp_path):
    from scipy.io import wavfile
    from gansynth_amd import reverb
    rng = np.random.default_rng(5)
    mono = (rng.standard_normal(300) * np.exp(-np.arange(300) / 60.0) * 9000).astype(np.int16)
    wavfile.write(str(tmp_path / "mono.wav"), 16000, mono)
    h = reverb.read_impulse(str(tmp_path / "mono.wav"), 16000)
    want = mono.astype(np.float64) / 32768.0
    assert tuple(h.shape) == (1, 300) and h.dtype == torch.float32
    assert np.array_equal(h.numpy()[0], (want / np.sqrt((want * want).sum())).astype(np.float32))
    delayed = reverb.read_impulse(str(tmp_path / "mono.wav"), 16000, predelay=0.001)
    assert tuple(delayed.shape) == (1, 316) and (delayed[:, :16] == 0).all() and torch.equal(delayed[:, 16:], h)
    stereo = (rng.standard_normal((200, 2)) * np.exp(-np.arange(200) / 40.0)[:, None] * [0.5, 0.25]).astype(np.float32)
    wavfile.write(str(tmp_path / "stereo.wav"), 48000, stereo)
    h2 = reverb.read_impulse(str(tmp_path / "stereo.wav"), 48000)
    s64 = stereo.T.astype(np.float64)
    norms = np.sqrt((s64 * s64).sum(axis=1))
    assert tuple(h2.shape) == (2, 200) and np.array_equal(h2.numpy(), (s64 / norms.max()).astype(np.float32))
    got = np.sqrt((h2.numpy().astype(np.float64) ** 2).sum(axis=1))
    assert abs(got[0] - 1) <= 2.0 ** -23 and abs(got[1] - norms[1] / norms[0]) <= 2.0 ** -23          # ONE factor: the balance stays
    wide = (rng.standard_normal((50, 2)) * (1 << 28)).astype(np.int32)
    wavfile.write(str(tmp_path / "wide.wav"), 44100, wide)
    w64 = wide.T.astype(np.float64) / 2147483648.0
    assert np.array_equal(reverb.read_impulse(str(tmp_path / "wide.wav"), 44100).numpy(), (w64 / np.sqrt((w64 * w64).sum(axis=1)).max()).astype(np.float32))
    wavfile.write(str(tmp_path / "three.wav"), 16000, np.zeros((10, 3), dtype=np.int16))
    with pytest.raises(ValueError, match="three.wav has 3 channels"):
        reverb.read_impulse(str(tmp_path / "three.wav"), 16000)
    wavfile.write(str(tmp_path / "empty.wav"), 16000, np.zeros((0,), dtype=np.int16))
    with pytest.raises(ValueError, match="empty.wav holds no samples"):
        reverb.read_impulse(str(tmp_path / "empty.wav"), 16000)
    wavfile.write(str(tmp_path / "silent.wav"), 16000, np.zeros((10,), dtype=np.int16))
    with pytest.raises(ValueError, match="all zero"):
        reverb.read_impulse(str(tmp_path / "silent.wav"), 16000)
    wavfile.write(str(tmp_path / "bytes.wav"), 16000, np.full((10,), 130, dtype=np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        reverb.read_impulse(str(tmp_path / "bytes.wav"), 16000)


@pytest.mark.parametrize("case", RV.cases(), ids=lambda c: "n%d-m%d-rows%d-ir%d" % c)
def test_fp32_restatement_leaves_the_kernel_room(case):
    """convolve_f32 -- the kernel's algorithm by another single-precision FFT -- stays inside a quarter of the tolerance the GPU test holds
    the kernel to, on the GPU test's own inputs; and the bound is not vacuous: it is below 2^-20 of the scale (16 fp32 roundings) on every case."""
    x, h = RV.draw(*case)
    ref, a = RV.convolve(x, h, RV.DRY, RV.WET), RV.scale(x, h, RV.DRY, RV.WET)
    e = RV.error(RV.convolve_f32(x, h, RV.DRY, RV.WET), ref, a)
    print(f"case {case}: e(convolve_f32) = {e:.4g}, recorded {RV.E_F32[case]:.4g}, tolerance {RV.tolerance(case):.4g}")
    assert 0 < e <= RV.tolerance(case) / 4 == RV.E_F32[case]
    assert RV.tolerance(case) < 2.0 ** -20


def test_reference_helpers():
    """The float64 convolution against the sum written out, the shared impulse, A, and finish's rule on a clip that clips."""
    x, h = RV.draw(37, 9, 2, 2)
    ref = RV.convolve(x, h, 0.5, 2.0)
    direct = np.stack([0.5 * np.concatenate([x[r].astype(np.float64), np.zeros(8)]) + 2.0 * np.convolve(x[r].astype(np.float64), h[r].astype(np.float64))
                       for r in range(2)])
    assert ref.shape == (2, 45) and np.abs(ref - direct).max() < 1e-14
    assert np.abs(RV.convolve(x, h[:1], 0.5, 2.0)[1] - (0.5 * np.concatenate([x[1].astype(np.float64), np.zeros(8)])
                                                        + 2.0 * np.convolve(x[1].astype(np.float64), h[0].astype(np.float64)))).max() < 1e-14
    assert (RV.scale(x, h, -0.5, 2.0) >= np.abs(RV.convolve(x, h, -0.5, 2.0)) - 1e-14).all()
    y = np.array([[0.5, -2.0, 1.0], [0.25, 1.5, -1.0]], dtype=np.float32)
    peak, out, pcm = RV.finish(y, True)
    assert peak == 2.0 and np.array_equal(out, y / 2) and pcm.shape == (3, 2) and pcm.tolist() == [[8192, 4096], [-32768, 24576], [16384, -16384]]
    peak, out, pcm = RV.finish(y, False)
    assert peak == 2.0 and np.array_equal(out, y) and pcm.tolist() == [[16384, 8192], [-32768, 32767], [32767, -32768]]
    peak, out, pcm = RV.finish(y[1] * np.float32(0.5), True)
    assert peak == 0.75 and out.shape == (1, 3) and pcm.shape == (3,) and pcm.tolist() == [4096, 24576, -16384]


def test_driver_flags():
    import gan_synth_main as main
    args = main.parser.parse_args(["--synthesize", "score.mid"])
    assert (args.reverb, args.reverb_ir, args.reverb_mix, args.reverb_predelay) == (None, None, 0.25, 0.0) and main.check_reverb_args(args) is False
    assert main.check_reverb_args(main.parser.parse_args([])) is False
    args = main.parser.parse_args(["--synthesize", "a.mid", "--reverb", "1.8", "--reverb_mix", "0.3", "--reverb_predelay", "0.02"])
    assert (args.reverb, args.reverb_ir, args.reverb_mix, args.reverb_predelay) == (1.8, None, 0.3, 0.02) and main.check_reverb_args(args) is True
    args = main.parser.parse_args(["--synthesize", "a.mid", "--reverb_ir", "hall.wav"])
    assert (args.reverb, args.reverb_ir) == (None, "hall.wav") and main.check_reverb_args(args) is True
    for argv, message in ((["--synthesize", "a.mid", "--reverb", "1.0", "--reverb_ir", "hall.wav"], "exclude each other"),
                          (["--generate", "--reverb", "1.0"], "--synthesize only"), (["--train", "--reverb_ir", "hall.wav"], "--synthesize only"),
                          (["--synthesize", "a.mid", "--reverb_mix", "0.5"], "need --reverb or --reverb_ir"),
                          (["--synthesize", "a.mid", "--reverb_predelay", "0.01"], "need --reverb or --reverb_ir"),
                          (["--synthesize", "a.mid", "--reverb", "0"], "positive RT60"), (["--synthesize", "a.mid", "--reverb", "-1"], "positive RT60"),
                          (["--synthesize", "a.mid", "--reverb", "1", "--reverb_mix", "1.5"], "reverb_mix must be in"),
                          (["--synthesize", "a.mid", "--reverb", "1", "--reverb_predelay", "-0.5"], "reverb_predelay must not be negative")):
        with pytest.raises(SystemExit, match=message):
            main.check_reverb_args(main.parser.parse_args(argv))
    with pytest.raises(SystemExit, match="--synthesize only"):     # main refuses before it touches a device
        main.main(main.parser.parse_args(["--generate", "--reverb", "1.0"]))
    with pytest.raises(SystemExit):
        main.parser.parse_args(["--reverb", "long"])
