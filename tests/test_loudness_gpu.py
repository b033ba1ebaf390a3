"""GPU: gs_loudness (gansynth_amd/csrc/loudness.hip) against the float64 rule of tests/loudness_ref.py, within 4 times the error of that file's
sequential fp32 restatement on the same input (R.FACTOR: the project's margin, not tuned to the kernel) -- at 16, 44.1 and 48 kHz, at the
lengths {hop - 1 (no hop: nothing written), hop, hop + 1, 4 hop, 4 hop + 1, 3 hop + 5, 2 s} (the kernel's tile IS a hop; two seconds carry
the state across 20 hops and thousands of chunks), one and two rows, row strides that put the rows on and off 16 bytes, NaN in the stride
padding of x and a sentinel around the energies; on noise over a DC offset, a constant, a second of silence before a burst and steps on
each side of every tile seam (R.master); and at 48010, 96000 and 192000 Hz, where the entry point takes its instantiation for long hops.
The exact properties -- two calls identical, rows independent, exact zeros before the first non-zero sample and for an all-zero clip, a
NaN confined to its row and to the hops from its own on -- hold bit for bit.  Then the Python layer, loudness.apply and the driver's
--loudness on the reduced PGGAN of tests/test_notes_gpu.py.
Every figure is printed before it is asserted."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

from tests import loudness_ref as R

pytestmark = pytest.mark.gpu
SENTINEL, PAD = 12345.0, 16


def _K():
    from gansynth_amd import kernels
    return kernels.get()


def _run(x, rate, aligned=True):
    """gs_loudness itself on x [rows, n]: x inside a buffer whose stride padding is NaN, the energies inside a buffer full of a sentinel.
    `aligned`: row strides that are multiples of 4 floats on 16-byte bases.  Else strides of 1 mod 4 floats -- row 1 is off 16 bytes -- and a
    single row moved off by one float.  -> energy [rows, hops] on the host; nothing outside it was written."""
    from gansynth_amd import kernels
    K = _K()
    lib, design = K.lib, K.loudness_design(rate)
    rows, n = x.shape
    hops = n // design.hop
    assert lib.gs_loudness_hops(ctypes.byref(design), n) == hops
    offset = 1 if (rows == 1 and not aligned) else 0
    stride = (n + 7) // 4 * 4 + (0 if aligned else 1)
    xbuf = torch.full((offset + rows * stride,), float("nan"), device="cuda")
    xv = xbuf[offset:].view(rows, stride)
    xv[:, :n] = torch.tensor(np.array(x), device="cuda")
    estride = hops + 3
    ebuf = torch.full((PAD + rows * estride + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    ev = ebuf[PAD:PAD + rows * estride].view(rows, estride)
    ws = torch.empty(max(int(lib.gs_loudness_workspace_bytes(ctypes.byref(design), rows, n)), 16), dtype=torch.uint8, device="cuda")
    assert (xv.data_ptr() % 16 == 0) == (offset == 0)
    code = lib.gs_loudness(ctypes.byref(design), xv.data_ptr(), rows, n, stride, ev.data_ptr(), estride, ws.data_ptr(), ws.numel(), kernels._stream())
    torch.cuda.synchronize()
    assert code == 0, lib.gs_last_error()
    assert (ebuf[:PAD] == SENTINEL).all() and (ebuf[PAD + rows * estride:] == SENTINEL).all() and (ev[:, hops:] == SENTINEL).all()
    return ev[:, :hops].cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "off16"])
@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("rate,n", [(rate, n) for rate in R.RATES for n in R.lengths(rate)], ids=lambda v: str(v))
def test_against_the_rule(rate, n, rows, aligned):
    hop = R.hop_of(rate)
    hops = n // hop
    refs = R.master_energies(rate)
    for kind in R.KINDS:
        x = R.master(rate, kind)[:rows, :n]
        z64, z32 = (z[:rows, :hops] for z in refs[kind])
        got = _run(x, rate, aligned)
        assert got.shape == (rows, hops) and got.dtype == np.float32
        e, b = R.error(got, z64), R.error(z32, z64)
        print(f"rate {rate} n {n} rows {rows} {'aligned' if aligned else 'off16'} {kind}: e(kernel) {e:.3g} against e(fp32) {b:.3g} "
              f"(ratio {e / b if b else 0:.3f})")
        assert e <= R.FACTOR * b
        if kind == "silence_burst":     # the hops before the first non-zero sample: exactly 0
            first = [rate, rate + hop + 3]
            for r in range(rows):
                quiet = min(first[r] // hop, hops)
                assert not _bits(got[r, :quiet]).any() and (hops <= quiet or got[r, quiet] > 0)
        if kind == "dc_noise":          # two calls: bit-identical; row 0 of two rows: the one-row call
            assert np.array_equal(_bits(_run(x, rate, aligned)), _bits(got))
            if rows == 2:
                assert np.array_equal(_bits(_run(x[:1], rate, aligned)[0]), _bits(got[0]))


@pytest.mark.parametrize("rate", [48010, 96000, 192000])
def test_the_instantiation_for_long_hops(rate):
    """Above 48 kHz a hop no longer fits the small LDS image and the entry point takes its second instantiation: the first rate beyond the
    threshold (hop 4801), one in the middle, and the highest rate, whose hop of 19200 fills the image to its last float."""
    hop = R.hop_of(rate)
    n = 3 * hop + 5
    g = np.random.Generator(np.random.PCG64(rate))
    x = (g.uniform(-0.25, 0.25, (2, n)) + np.array([[0.6], [-0.45]])).astype(np.float32)
    z64, z32 = R.energy_f64(x, rate), R.energy_f32(x, rate)
    b = R.error(z32, z64)
    for aligned in (True, False):
        got = _run(x, rate, aligned)
        e = R.error(got, z64)
        print(f"rate {rate} hop {hop} n {n} {'aligned' if aligned else 'off16'}: e(kernel) {e:.3g} against e(fp32) {b:.3g} (ratio {e / b:.3f})")
        assert e <= R.FACTOR * b
        assert np.array_equal(_bits(_run(x[:1], rate, aligned)[0]), _bits(got[0]))


@pytest.mark.parametrize("rate", R.RATES)
def test_all_zero_input_gives_all_zero_energies(rate):
    n = 5 * R.hop_of(rate) + 9
    for aligned in (True, False):
        got = _run(np.zeros((2, n), dtype=np.float32), rate, aligned)
        assert got.shape == (2, 5) and not _bits(got).any()


@pytest.mark.parametrize("rate", R.RATES)
@pytest.mark.parametrize("where", ["first sample", "seam", "mid hop"])
def test_a_nan_stays_in_its_row_and_behind_itself(rate, where):
    hop = R.hop_of(rate)
    n = 6 * hop + 11
    at = {"first sample": 0, "seam": 2 * hop, "mid hop": 3 * hop + hop // 2}[where]
    x = R.master(rate, "dc_noise")[:, :n].copy()
    x[1, at] = np.nan
    for aligned in (True, False):
        got = _run(x, rate, aligned)                                   # (status 0 is asserted there)
        alone = _run(x[:1], rate, aligned)
        assert np.array_equal(_bits(got[0]), _bits(alone[0])) and np.isfinite(got[0]).all()
        clean = _run(R.master(rate, "dc_noise")[:, :n], rate, aligned)
        assert np.array_equal(_bits(got[1, :at // hop]), _bits(clean[1, :at // hop])) and np.isnan(got[1, at // hop:]).all()


def test_the_python_layer():
    from gansynth_amd import kernels, loudness
    K = _K()
    rate, hop = 48000, 4800
    x = R.master(rate, "dc_noise")[:, :5 * hop + 77]
    xd = torch.tensor(np.array(x), device="cuda")
    got = kernels.loudness_energy(xd, rate)
    assert got.shape == (2, 5) and got.dtype == torch.float32 and got.is_cuda
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(_run(x, rate)))
    mono = K.loudness_energy(xd[1], rate)
    assert mono.shape == (1, 5) and np.array_equal(_bits(mono.cpu().numpy()), _bits(_run(x[1:], rate)))
    wide = torch.full((2, 5 * hop + 78), float("nan"), device="cuda")                     # a view with rows off 16 bytes: taken as it is
    wide[:, :5 * hop + 77] = xd
    assert torch.equal(K.loudness_energy(wide[:, :5 * hop + 77], rate), got)
    assert torch.equal(K.loudness_energy(xd.t().contiguous().t(), rate), got)             # samples not contiguous: copied
    assert K.loudness_energy(xd[:, :hop - 1], rate).shape == (2, 0)                       # no complete hop
    assert K.loudness_design(rate) is K.loudness_design(rate)                             # one design a rate
    with pytest.raises(ValueError, match="must be on the HIP device"):
        K.loudness_energy(xd.cpu(), rate)
    # measure: the gating on the kernel's energies against the float64 rule end to end
    long = np.array(R.master(rate, "silence_burst"))
    lufs, want = loudness.measure(torch.tensor(long, device="cuda"), rate), R.lufs_of(long, rate)
    print(f"measure: {lufs:.6f} LUFS against {want:.6f} by the float64 rule")
    assert abs(lufs - want) <= 1e-4
    assert loudness.measure(torch.zeros(2, rate, device="cuda"), rate) == -math.inf
    assert loudness.measure(xd[0, :3 * hop], rate) == -math.inf                            # fewer than 4 hops
    bad = xd.clone()
    bad[0, 100] = float("inf")
    with pytest.raises(ValueError, match="not all finite"):
        loudness.measure(bad, rate)


def _two_levels(rate, seconds=3):
    """Noise at two levels 6.9 LU apart, both channels: every gating block is far from both gates."""
    n = seconds * rate
    g = np.random.default_rng(8)
    env = np.where(np.arange(n) < n // 2, 1.0, 0.45)
    return (g.uniform(-0.6, 0.6, (2, n)) * env).astype(np.float32)


@pytest.mark.parametrize("rate", [48000, 44100])
def test_apply_meets_the_target_where_the_limiter_rests(rate):
    from gansynth_amd import kernels, loudness
    x = _two_levels(rate)
    hop = R.hop_of(rate)
    margin, before = R.gate_margin(R.energy_f64(x, rate), hop), R.lufs_of(x, rate)
    assert margin > 0.5, margin
    target = -30.0
    out, pcm, info = loudness.apply(torch.tensor(x, device="cuda"), rate, target, want_pcm=True)
    after = R.lufs_of(out.cpu().numpy(), rate)
    print(f"apply at {rate}: {before:.4f} LUFS by the rule, measured {info['measured_lufs']:.4f}, pre_gain {info['pre_gain']:.6f}, out {after:.4f} by the "
          f"rule ({info['output_lufs']:.4f} measured) for a target of {target}, least gain {info['min_gain']}, peak {info['peak']:.4f}, gate margin {margin:.2f} LU")
    assert info["min_gain"] == 1.0 and abs(after - target) <= 0.01 and abs(info["output_lufs"] - after) <= 1e-3
    assert abs(info["measured_lufs"] - before) <= 1e-3 and info["pre_gain"] == 10.0 ** ((target - info["measured_lufs"]) / 20.0)
    assert out.shape == (2, x.shape[1]) and pcm.shape == (x.shape[1], 2) and pcm.dtype == torch.int16
    want = kernels.limit(torch.tensor(x, device="cuda"), info["pre_gain"], 10.0 ** (-1.0 / 20), int(math.floor(0.005 * rate + 0.5)), want_pcm=True)
    assert torch.equal(out, want[0]) and torch.equal(pcm, want[1]) and info["peak"] == float(want[2])
    # a target the ceiling does not allow: the limiter works, no sample passes the ceiling, the output falls short
    loud = before + 6.0                                # 6 dB up: the peak of 0.6 would stand at 1.2, over the ceiling of 0.891
    _, _, hot = loudness.apply(torch.tensor(x, device="cuda"), rate, loud)
    print(f"apply at {rate}, target {loud:.3f}: out {hot['output_lufs']:.3f} LUFS, least gain {hot['min_gain']:.4f}, peak {hot['peak']:.6f}")
    assert hot["min_gain"] < 1 and hot["peak"] <= np.float32(10.0 ** (-1.0 / 20)) and hot["output_lufs"] < loud
    # silence keeps its gain of 1
    _, _, still = loudness.apply(torch.zeros(2, rate, device="cuda"), rate, -23.0)
    assert still["measured_lufs"] == -math.inf and still["pre_gain"] == 1.0 and still["output_lufs"] == -math.inf and still["peak"] == 0.0


# ---------------------------------------------------------------------------------------------------------------- the driver
def _score():
    """Fourteen overlapping notes over 0.65 s: the reduced model's notes last 64 ms, and a measurement needs 400 ms."""
    return [dict(pitch=48 + (7 * i) % 25, velocity=80 + (11 * i) % 40, start=round(0.045 * i, 3), end=round(0.045 * i + 0.05, 3),
                 pan=round(-0.6 + 0.09 * i, 2)) for i in range(14)]


def test_driver_loudness(gpu_store, tmp_path):
    """`gan_synth_main.py --synthesize score.json --stereo --output_rate 48000 --loudness -30` after building its model: the written WAV,
    measured by the float64 rule, lies within the meter tolerance of 0.1 LU of -30; `--loudness -8` drives the limiter (least gain below 1, no
    sample beyond round(c * 32768)); and without the flag the file is the one model.synthesize quantises itself, as before."""
    from scipy.io import wavfile
    import gan_synth_main as main
    from tests.test_notes_gpu import _model
    model = _model()
    (tmp_path / "score.json").write_text(json.dumps(_score()))
    common = ["--synthesize", str(tmp_path / "score.json"), "--batch_size", "4", "--release_seconds", "0.01", "--model_dir", str(tmp_path / "no_model"),
              "--seed", "3", "--stereo", "--output_rate", "48000"]
    c = 10.0 ** (-1.0 / 20)
    lines = []

    def render(name, extra):
        args = main.parser.parse_args(common + ["--output", str(tmp_path / name)] + extra)
        info = main.synthesize_to_wav(model, args, range(24, 85), log=lines.append)
        rate, data = wavfile.read(str(tmp_path / name))
        assert rate == 48000 and data.dtype == np.int16 and data.ndim == 2 and data.shape[1] == 2
        return info, data

    info, data = render("target.wav", ["--loudness", "-30"])
    heard = R.lufs_of(data.T.astype(np.float64) / 32768.0, 48000)
    print(f"driver --loudness -30: {data.shape[0]} samples, measured {info['loudness_measured']:.3f} LUFS before, {info['loudness_output']:.3f} after, the file "
          f"{heard:.3f} LUFS by the float64 rule, least gain {info['limit_min_gain']}")
    assert data.shape[0] >= 4 * 4800 and abs(heard + 30.0) <= 0.1
    assert info["loudness_target"] == -30.0 and math.isfinite(info["loudness_measured"]) and abs(info["loudness_output"] + 30.0) <= 0.1
    assert info["limit_ceiling_db"] == -1.0 and "limit_drive_db" not in info
    written = [line for line in lines if "written to" in line]
    assert "for a target of -30 under a ceiling of -1 dBFS" in written[-1] and "limited to" not in written[-1]
    assert ("short of the target" in written[-1]) == (info["limit_min_gain"] < 1)
    # a target the ceiling does not allow
    hot_info, hot = render("hot.wav", ["--loudness", "-8", "--limit", "-1", "--limit_lookahead", "0.002"])
    print(f"driver --loudness -8: largest |pcm| {np.abs(hot.astype(np.int64)).max()} against round(c * 32768) = {round(c * 32768)}, least gain "
          f"{hot_info['limit_min_gain']:.4f}, output {hot_info['loudness_output']:.3f} LUFS")
    assert hot_info["limit_min_gain"] < 1 and np.abs(hot.astype(np.int64)).max() <= round(c * 32768) and hot_info["limit_peak"] <= np.float32(c)
    assert hot_info["loudness_output"] < -8.0 and "short of the target" in [line for line in lines if "written to" in line][-1]
    # without the flag: the file of the chain as it was (model.synthesize normalising and quantising)
    plain_info, plain = render("plain.wav", [])
    assert "loudness_target" not in plain_info and "limit_min_gain" not in plain_info and "LUFS" not in lines[-1]
    _, pcm = model.synthesize(str(tmp_path / "score.json"), want_pcm=True, sample_rate=48000, stereo=True, batch_size=4, release_seconds=0.01, seed=3)
    assert np.array_equal(plain, pcm.cpu().numpy())
