"""CPU: the output-rate rule (DESIGN.md "Output rates") without a device -- gs_resample_design / _out_len / _table against the float64
restatement of tests/resample_ref.py, every refusal of the entry points (no launch), the quality of the rule itself (DC, passband,
stopband, overshoot), the descriptor's ctypes mirror, `--output_rate` and the equal-rates shortcut of spectral_ops.resample."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import resample_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the issue's table: (rate_in, rate_out) -> (up, down, taps)
DESIGNS = {(16000, 48000): (3, 1, 68), (16000, 44100): (441, 160, 68), (44100, 16000): (160, 441, 186), (48000, 16000): (1, 3, 204),
           (16000, 22050): (441, 320, 68)}


def _lib_and_design(rate_in, rate_out):
    from gansynth_amd import _lib
    lib = _lib.load()
    d = _lib.GsResample()
    assert lib.gs_resample_design(rate_in, rate_out, ctypes.byref(d)) == 0, lib.gs_last_error()
    return _lib, lib, d


@pytest.fixture(scope="module")
def tables():
    """(rate_in, rate_out) -> the float64 reference table, computed once."""
    return {pair: RR.table(*RR.design(*pair)) for pair in RR.PAIRS}


def test_design_and_output_length():
    assert sorted(RR.PAIRS) == sorted(DESIGNS)
    for (rate_in, rate_out), want in DESIGNS.items():
        _, lib, d = _lib_and_design(rate_in, rate_out)
        assert (d.up, d.down, d.taps) == want == RR.design(rate_in, rate_out), (rate_in, rate_out)
        assert (d.rate_in, d.rate_out, d.zeros) == (rate_in, rate_out, RR.ZEROS)
        for n_in in (1, 2, 7, 160, 441, 5000, 64000, 13600000, 1 << 40):
            assert lib.gs_resample_out_len(ctypes.byref(d), n_in) == -(-n_in * d.up // d.down) == RR.out_len(n_in, d.up, d.down)
        assert lib.gs_resample_out_len(ctypes.byref(d), 1) == (d.up + d.down - 1) // d.down >= 1
    _, lib, d = _lib_and_design(16000, 48000)
    assert lib.gs_resample_out_len(ctypes.byref(d), 64000) == 192000
    _, lib, d = _lib_and_design(16000, 44100)
    assert lib.gs_resample_out_len(ctypes.byref(d), 1024) == 2823     # ceil(1024 * 441 / 160)


def test_descriptor_mirror_and_constants():
    from gansynth_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gansynth_hip.h")).read()
    assert int(re.search(r"#define GS_RESAMPLE_TILE (\d+)", hdr).group(1)) == _lib.RESAMPLE_TILE
    assert int(re.search(r"#define GS_RESAMPLE_ZEROS (\d+)", hdr).group(1)) == RR.ZEROS
    assert float(re.search(r"#define GS_RESAMPLE_ROLLOFF ([0-9.]+)", hdr).group(1)) == RR.ROLLOFF
    assert float(re.search(r"#define GS_RESAMPLE_BETA ([0-9.]+)", hdr).group(1)) == RR.BETA
    assert ctypes.sizeof(_lib.GsResample) == 24
    assert [(n, getattr(_lib.GsResample, n).offset) for n, _ in _lib.GsResample._fields_] == \
        [("rate_in", 0), ("rate_out", 4), ("up", 8), ("down", 12), ("taps", 16), ("zeros", 20)]


def test_table_against_the_reference(tables):
    for pair in RR.PAIRS:
        _, lib, d = _lib_and_design(*pair)
        ref = tables[pair]
        assert lib.gs_resample_table_bytes(ctypes.byref(d), 0) == d.up * d.taps * 4
        got = np.full((d.up, d.taps), np.nan, dtype=np.float32)
        assert lib.gs_resample_table(ctypes.byref(d), 0, got.ctypes.data) == 0
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= 2.0 ** -23 * np.abs(ref) + 1e-12).all(), (pair, float(err.max()))
        # the layout gs_resample reads: the same rows, padded with zeros to a multiple of four coefficients
        row = (d.taps + 3) & ~3
        assert lib.gs_resample_table_bytes(ctypes.byref(d), 1) == d.up * row * 4
        dev = np.full((d.up, row), np.nan, dtype=np.float32)
        assert lib.gs_resample_table(ctypes.byref(d), 1, dev.ctypes.data) == 0
        assert np.array_equal(dev[:, :d.taps], got) and np.array_equal(dev[:, d.taps:], np.zeros((d.up, row - d.taps), dtype=np.float32))
    assert (186 + 3) & ~3 == 188     # (44100 -> 16000 is the pair whose rows need the padding)


def test_refusals_without_gpu():
    from gansynth_amd import _lib
    lib = _lib.load()
    d = _lib.GsResample()
    for rate_in, rate_out, message in ((0, 16000, b"positive"), (16000, 0, b"positive"), (-16000, 48000, b"positive"), (16000, -1, b"positive"),
                                       (16000, 16000, b"equal"), (16000, 44101, b"up ="), (16000, 1025 * 16000, b"up ="),
                                       (16000, 1000, b"taps ="), (48000, 3000, b"taps =")):
        assert lib.gs_resample_design(rate_in, rate_out, ctypes.byref(d)) == -1, (rate_in, rate_out)       # GS_ERR_ARG
        assert message in lib.gs_last_error(), (rate_in, rate_out, lib.gs_last_error())
    assert lib.gs_resample_design(16000, 48000, None) == -1 and b"null" in lib.gs_last_error()
    assert lib.gs_resample_design(16000, 1100, ctypes.byref(d)) == 0 and d.taps <= 1024           # (a ratio of 14.5 is still served)

    _, lib, d = _lib_and_design(44100, 16000)
    P = 0x10000   # (never dereferenced: the argument checks come first and nothing is launched)
    good = dict(r=ctypes.byref(d), table=P, x=P, rows=3, n_in=5000, row_stride=5003, normalize=1, out=P, pcm=None, peak=None, ws=P,
                ws_bytes=1 << 20, stream=None)
    order = ["r", "table", "x", "rows", "n_in", "row_stride", "normalize", "out", "pcm", "peak", "ws", "ws_bytes", "stream"]
    bad = [("rows", 0, b"rows"), ("rows", -1, b"rows"), ("n_in", 0, b"n_in"), ("n_in", -7, b"n_in"), ("row_stride", 4999, b"row_stride"),
           ("x", None, b"null"), ("out", None, b"null"), ("table", None, b"null"), ("ws_bytes", 8, b"workspace"), ("ws", None, b"workspace"),
           ("r", None, b"descriptor"), ("table", P + 4, b"misaligned"), ("out", P + 2, b"misaligned")]
    for field, value, message in bad:
        args = dict(good, **{field: value})
        assert lib.gs_resample(*[args[k] for k in order]) == -1, (field, value)
        assert message in lib.gs_last_error(), (field, value, lib.gs_last_error())
    # a descriptor that does not follow from its rates, one field at a time -- and rates no design exists for
    for field, value, message in (("up", 161, b"does not follow"), ("down", 440, b"does not follow"), ("taps", 188, b"does not follow"),
                                  ("taps", 184, b"does not follow"), ("zeros", 16, b"does not follow"), ("rate_out", 44100, b"equal"),
                                  ("rate_in", 0, b"positive"), ("rate_out", 16001, b"up =")):
        wrong = _lib.GsResample(d.rate_in, d.rate_out, d.up, d.down, d.taps, d.zeros)
        setattr(wrong, field, value)
        assert lib.gs_resample(*[dict(good, r=ctypes.byref(wrong))[k] for k in order]) == -1, (field, value)
        assert message in lib.gs_last_error(), (field, value, lib.gs_last_error())
        assert lib.gs_resample_out_len(ctypes.byref(wrong), 5000) == -1
        assert lib.gs_resample_table_bytes(ctypes.byref(wrong), 0) == 0 and lib.gs_resample_workspace_bytes(ctypes.byref(wrong), 1, 5000) == 0
        assert lib.gs_resample_table(ctypes.byref(wrong), 0, P) == -1
    assert lib.gs_resample_table(ctypes.byref(d), 0, None) == -1 and b"null" in lib.gs_last_error()
    nbytes = lib.gs_resample_workspace_bytes
    n_out = -(-5000 * 160 // 441)
    assert nbytes(ctypes.byref(d), 3, 5000) == 3 * 4 * -(-n_out // _lib.RESAMPLE_TILE)
    assert nbytes(ctypes.byref(d), 1, 1) == 4 and nbytes(ctypes.byref(d), 0, 5000) == 0 and nbytes(ctypes.byref(d), 3, 0) == 0
    assert lib.gs_resample_out_len(ctypes.byref(d), 0) == -1 and lib.gs_resample_out_len(ctypes.byref(d), (1 << 40) + 1) == -1


# ------------------------------------------------------------------------------------------ the quality of the rule itself (float64)
def _tone(n, cycles_per_sample, phase=0.3):
    return np.sin(2 * np.pi * cycles_per_sample * np.arange(n) + phase)


def test_dc_gain_of_every_phase(tables):
    """A constant input comes out constant: no phase's coefficients sum further than 1e-6 from 1 (measured: 4.6e-7), which is why the
    rule has no per-phase renormalisation."""
    for pair in RR.PAIRS:
        assert np.abs(tables[pair].sum(axis=1) - 1.0).max() <= 1e-6, pair


def test_row_sums_show_the_overshoot(tables):
    """sum_k |T[p][k]| reaches 2.37: a clip normalised to |x| <= 1 can leave the filter above 1, hence the normalisation behind it."""
    worst = max(float(np.abs(tables[pair]).sum(axis=1).max()) for pair in RR.PAIRS)
    assert 2.0 < worst <= 2.37, worst


def test_passband(tables):
    """Sines at 0.05 - 0.85 of the lower Nyquist come out as the same sine at the new rate, interior samples within 5e-4 (measured: 2.2e-4)."""
    for pair in [(16000, 48000), (16000, 44100), (44100, 16000), (48000, 16000)]:
        up, down, taps = RR.design(*pair)
        n_in = 4000
        lower_nyquist = 0.5 * min(1.0, up / down)                         # cycles per INPUT sample
        worst = 0.0
        for fraction in (0.05, 0.25, 0.5, 0.7, 0.85):
            f = fraction * lower_nyquist
            y, _ = RR.resample(_tone(n_in, f), tables[pair], up, down)
            j = np.arange(y.shape[0])
            want = np.sin(2 * np.pi * f * (j * down / up) + 0.3)          # output j sits at input time j * down / up
            interior = (j * down / up > taps) & (j * down / up < n_in - taps)
            assert interior.sum() > 500
            worst = max(worst, float(np.abs(y - want)[interior].max()))
        assert worst <= 5e-4, (pair, worst)


def test_stopband(tables):
    """Downsampling: sines at 1.06 - 2.0 times the NEW Nyquist, which would alias, come out below 5e-5 (measured: 1.4e-5)."""
    for pair in [(44100, 16000), (48000, 16000)]:
        up, down, taps = RR.design(*pair)
        n_in = 6000
        new_nyquist = 0.5 * up / down                                     # cycles per input sample
        worst = 0.0
        for factor in (1.06, 1.2, 1.5, 2.0):
            y, _ = RR.resample(_tone(n_in, factor * new_nyquist), tables[pair], up, down)
            t = np.arange(y.shape[0]) * down / up
            interior = (t > taps) & (t < n_in - taps)
            assert interior.sum() > 500
            worst = max(worst, float(np.abs(y)[interior].max()))
        assert worst <= 5e-5, (pair, worst)


def test_reference_edges_and_bound():
    """The restatement itself: indices outside the row contribute 0, B bounds |y|, and a faithful fp32 loop sits well inside the bound
    the kernel is held to."""
    up, down, taps = RR.design(16000, 44100)
    tab = RR.table(up, down, taps).astype(np.float32)
    x = (np.random.default_rng(3).random(300) * 2 - 1).astype(np.float32)
    y, b = RR.resample(x, tab, up, down)
    assert y.shape == (RR.out_len(300, up, down),) and (np.abs(y) <= b).all()
    padded = np.concatenate([np.zeros(taps), x.astype(np.float64), np.zeros(taps)])
    for j in (0, 1, 5, y.shape[0] // 2, y.shape[0] - 1):
        i0, p = j * down // up, j * down % up
        want = sum(float(tab[p, k]) * padded[taps + i0 - taps // 2 + 1 + k] for k in range(taps))
        assert abs(y[j] - want) <= 1e-12
    acc = np.zeros(y.shape[0], dtype=np.float32)
    j = np.arange(y.shape[0])
    i0, p = j * down // up, j * down % up
    xp = np.concatenate([np.zeros(taps, np.float32), x, np.zeros(taps, np.float32)])
    for k in range(taps):
        acc = (acc + (tab[p, k] * xp[taps + i0 - taps // 2 + 1 + k]).astype(np.float32)).astype(np.float32)
    ratio = np.abs(acc.astype(np.float64) - y) / RR.bound(b, taps)
    assert ratio.max() <= 0.25, float(ratio.max())


# ------------------------------------------------------------------------------------------------------------------ Python surface
def test_driver_parses_output_rate():
    import gan_synth_main as main
    assert main.parser.parse_args([]).output_rate is None
    args = main.parser.parse_args(["--synthesize", "score.mid", "--output_rate", "48000"])
    assert args.output_rate == 48000 and args.synthesize == "score.mid"
    assert main.parser.parse_args(["--generate", "--output_rate", "44100"]).output_rate == 44100
    with pytest.raises(SystemExit):
        main.parser.parse_args(["--output_rate", "fast"])


def test_equal_rates_return_the_argument():
    """No device is touched (this runs without one): the same object comes back."""
    from gansynth_amd import spectral_ops
    x = torch.zeros(2, 100)
    assert spectral_ops.resample(x, 16000, 16000) is x
    row = x[0]
    assert spectral_ops.resample(row, 44100, 44100) is row
    with pytest.raises(ValueError, match="positive"):
        spectral_ops.resample(x, 0, 16000)
    with pytest.raises(ValueError, match="positive"):
        spectral_ops.resample(x, 16000, -48000)


def test_synthesize_and_generate_take_sample_rate():
    import inspect
    from gansynth_amd.models import GANSynth
    assert inspect.signature(GANSynth.synthesize).parameters["sample_rate"].default is None
    for form in (GANSynth._generate_batch, GANSynth._generate_from):
        assert inspect.signature(form).parameters["sample_rate"].default is None
