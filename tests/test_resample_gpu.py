"""GPU: gs_resample against the float64 restatement of tests/resample_ref.py -- an impulse train that must return single table
coefficients bit for bit, random rows within the a-priori bound (taps + 3) * 2^-24 * B at EVERY output, the row ends and the tile
edges, outputs whose j * down passes 2^31, the peak / normalisation / PCM tail, determinism -- and the layers above it end to end on the
reduced PGGAN of tests/test_notes_gpu.py: GANSynth.synthesize / generate with sample_rate and the driver's --output_rate.

The reference for the bound uses the library's own fp32 table widened to double: the table's rounding is tests/test_resample_cpu.py's
matter, the kernel's arithmetic is this file's."""
import ctypes
import json

import numpy as np
import pytest
import torch

from oracle import torch_ref as R
from tests import resample_ref as RR

pytestmark = pytest.mark.gpu
TILE = 512


def _K():
    from gansynth_amd import kernels
    return kernels.get()


_TABLES = {}


def _design(pair):
    """(GsResample, the library's fp32 table [up, taps] widened to float64), once per pair."""
    from gansynth_amd import _lib
    if pair not in _TABLES:
        lib = _lib.load()
        d = _lib.GsResample()
        assert lib.gs_resample_design(pair[0], pair[1], ctypes.byref(d)) == 0
        tab = np.empty((d.up, d.taps), dtype=np.float32)
        assert lib.gs_resample_table(ctypes.byref(d), 0, tab.ctypes.data) == 0
        _TABLES[pair] = (d, tab.astype(np.float64))
    return _TABLES[pair]


def _check(got, x, pair, what, outputs=None):
    """Every output of every row within the bound of the float64 sum; returns the worst error / bound."""
    d, tab = _design(pair)
    got, x = np.atleast_2d(got), np.atleast_2d(x)
    worst = 0.0
    for r in range(x.shape[0]):
        y, b = RR.resample(x[r], tab, d.up, d.down, outputs=outputs)
        g = got[r] if outputs is None else got[r][outputs]
        assert g.shape == y.shape and g.dtype == np.float32, (what, g.shape, y.shape)
        err = np.abs(g.astype(np.float64) - y)
        bound = RR.bound(b, d.taps)
        bad = np.flatnonzero(~(err <= bound))          # (NaN fails)
        assert bad.size == 0, (what, r, len(bad), bad[:4].tolist(), g[bad[:4]].tolist(), y[bad[:4]].tolist())
        if (b > 0).any():
            worst = max(worst, float((err[b > 0] / bound[b > 0]).max()))
    print(f"{what}: worst error / bound = {worst:.3f}")
    return worst


@pytest.mark.parametrize("pair", [(16000, 48000), (16000, 44100), (44100, 16000)])
def test_impulse_train_returns_single_coefficients(pair):
    """1.0 every taps + 1 samples: no window of `taps` inputs holds two of them, so an output is ONE coefficient times 1.0 plus zeros --
    T[p][k] itself, bit for bit, with p and k from the rule (this pins lead and lag), or 0 where the window misses every impulse."""
    d, tab = _design(pair)
    n_in, period = 8192, d.taps + 1
    x = np.zeros(n_in, dtype=np.float32)
    x[::period] = 1.0
    out, _, _ = _K().resample(torch.from_numpy(x).cuda(), *pair)
    n_out = RR.out_len(n_in, d.up, d.down)
    assert tuple(out.shape) == (1, n_out)
    j = np.arange(n_out, dtype=np.int64)
    i0, p = j * d.down // d.up, j * d.down % d.up
    start = i0 - d.taps // 2 + 1                                  # the window is x[start .. start + taps)
    pos = -(-start // period) * period                            # the first multiple of the period at or behind its start
    hit = (pos < start + d.taps) & (pos >= 0) & (pos < n_in)
    want = np.where(hit, tab[p, np.clip(pos - start, 0, d.taps - 1)], 0.0).astype(np.float32)
    assert set(p.tolist()) == set(range(d.up)) and hit.sum() > 0.9 * n_out and (~hit).sum() > 0
    assert np.array_equal(out[0].cpu().numpy(), want)


@pytest.mark.parametrize("pair", RR.PAIRS)
def test_random_rows_with_padded_stride(pair):
    """rows = 3, n_in = 5000, rows 5003 apart and NaN between them: a tap that reaches into the padding or the next row contributes 0."""
    store = torch.full((3, 5003), float("nan"))
    store[:, :5000] = torch.rand(3, 5000, generator=torch.Generator().manual_seed(5)) * 2 - 1
    dev = store.cuda()
    x = dev[:, :5000]
    assert x.stride(0) == 5003
    out, _, _ = _K().resample(x, *pair)
    d, _ = _design(pair)
    assert tuple(out.shape) == (3, RR.out_len(5000, d.up, d.down))
    _check(out.cpu().numpy(), store[:, :5000].numpy(), pair, f"random rows {pair}")
    assert torch.equal(dev[:, 5000:].isnan(), torch.ones(3, 3, dtype=torch.bool, device="cuda"))


def _n_in_for(n_out, up, down):
    """An n_in with ceil(n_in * up / down) == n_out, or None (an upsampling ratio skips lengths)."""
    for n_in in range(max(1, (n_out - 2) * down // up - 2), n_out * down // up + 3):
        if RR.out_len(n_in, up, down) == n_out:
            return n_in
    return None


@pytest.mark.parametrize("pair", [(16000, 48000), (16000, 44100), (44100, 16000), (48000, 16000)])
def test_row_ends_and_tile_edges(pair):
    """Rows shorter than the filter (every window hangs over both ends), and output lengths one below, at and one above a multiple of
    the block tile (two multiples: a partial last block behind one and behind two full ones)."""
    d, _ = _design(pair)
    lengths = [1, 7, d.taps - 1]
    reached = []
    for n_out in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1):
        n_in = _n_in_for(n_out, d.up, d.down)
        if n_in is not None:
            lengths.append(n_in)
            reached.append(n_out)
    assert len(reached) >= (6 if d.up < d.down else 2), reached       # downsampling reaches every length
    rng = np.random.default_rng(9)
    for n_in in lengths:
        x = (rng.random((2, n_in)) * 2 - 1).astype(np.float32)
        out, pcm, peak = _K().resample(torch.from_numpy(x).cuda(), *pair, want_pcm=True)
        assert tuple(out.shape) == (2, RR.out_len(n_in, d.up, d.down)) == tuple(pcm.shape)
        got = out.cpu().numpy()
        _check(got, x, pair, f"{pair} n_in = {n_in}")
        assert np.array_equal(peak.cpu().numpy(), np.abs(got).max(axis=1)) and np.array_equal(pcm.cpu().numpy(), RR.pcm16(got))


def test_indices_beyond_32_bits():
    """44100 -> 16000 over 13.6 M samples: j * down passes 2^31 near j = 4.87 M.  The first and last 2048 outputs, 512 around the
    crossing and 4096 seeded random ones against the bound."""
    pair = (44100, 16000)
    d, _ = _design(pair)
    n_in = 13600000
    x = (np.random.default_rng(21).random(n_in, dtype=np.float32) * 2 - 1)
    out, _, peak = _K().resample(torch.from_numpy(x).cuda(), *pair)
    n_out = RR.out_len(n_in, d.up, d.down)
    assert tuple(out.shape) == (1, n_out) and (n_out - 1) * d.down > 2 ** 31
    crossing = 2 ** 31 // d.down
    assert 4860000 < crossing < 4880000 and crossing + 256 < n_out - 2048
    picks = np.unique(np.concatenate([np.arange(2048), np.arange(n_out - 2048, n_out), np.arange(crossing - 256, crossing + 256),
                                      np.random.default_rng(22).integers(0, n_out, 4096)]))
    got = out.cpu().numpy()
    _check(got, x, pair, "13.6 M samples", outputs=picks)
    assert float(peak[0]) == float(np.abs(got).max())


def _raw(pair, x, normalize, want_pcm, want_peak):
    """gs_resample itself: (return code, out, pcm, peak), the results prefilled so that an untouched one shows."""
    from gansynth_amd import kernels
    K = _K()
    d, table = K.resample_design(pair[0], pair[1], x.device)
    rows, n_in = x.shape
    n_out = RR.out_len(n_in, d.up, d.down)
    out = torch.full((rows, n_out), float("nan"), device="cuda")
    pcm = torch.full((rows, n_out), 77, dtype=torch.int16, device="cuda") if want_pcm else None
    peak = torch.full((rows,), -1.0, device="cuda") if want_peak else None
    ws = torch.empty(max(K.lib.gs_resample_workspace_bytes(ctypes.byref(d), rows, n_in), 256), dtype=torch.uint8, device="cuda")
    code = K.lib.gs_resample(ctypes.byref(d), table.data_ptr(), x.data_ptr(), rows, n_in, x.stride(0), 1 if normalize else 0, out.data_ptr(),
                             None if pcm is None else pcm.data_ptr(), None if peak is None else peak.data_ptr(), ws.data_ptr(), ws.numel(),
                             kernels._stream())
    torch.cuda.synchronize()
    return code, out, pcm, peak


def test_peak_normalisation_and_pcm():
    """One call, three rows, each finished by its OWN peak: a +-1 square wave, whose band-limited interpolation overshoots 1, a quiet row
    that is left alone, and a loud sine with another peak above 1.  The input rows lie 4006 apart (a padded stride that 4 does not
    divide) and n_out = 12003 (n_out % 4 == 3), so the second and third row of out and of pcm start off the 16-byte grid: the wide form
    of the second launch runs on the first row and the sample-by-sample form on the others, a 3-sample tail behind each."""
    K = _K()
    pair = (16000, 48000)
    n_in = 4001
    t = np.arange(n_in)
    x = np.stack([np.where((t // 25) % 2 == 0, 1.0, -1.0), 0.25 * np.sin(0.05 * t), 1.75 * np.sin(0.03 * t)]).astype(np.float32)
    store = torch.full((3, 4006), float("nan"))
    store[:, :n_in] = torch.from_numpy(x)
    dev = store.cuda()[:, :n_in]
    assert dev.stride(0) == 4006
    y, none, peak0 = K.resample(dev, *pair)
    assert none is None and tuple(y.shape) == (3, 12003) and y.shape[1] % 4 == 3 and y[1].data_ptr() % 16 != 0 and y[2].data_ptr() % 16 != 0
    _check(y.cpu().numpy(), x, pair, "square wave")
    exact = y.abs().max(dim=1).values
    assert torch.equal(peak0, exact) and float(exact[0]) > 1.0 and float(exact[1]) <= 0.5     # a maximum is exact
    assert float(exact[2]) > 1.5 and float(exact[2]) != float(exact[0])                      # (a row's peak is its own)
    out, pcm, peak = K.resample(dev, *pair, normalize=True, want_pcm=True)
    assert torch.equal(peak, exact)                                                             # the peak of y, not of out
    yn, on = y.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(on[0], yn[0] / np.float32(exact[0].item()))                            # IEEE division: correctly rounded
    assert np.array_equal(on[1], yn[1]) and float(np.abs(on[0]).max()) == 1.0                    # the quiet row is left alone
    assert np.array_equal(on[2], yn[2] / np.float32(exact[2].item())) and float(np.abs(on[2]).max()) == 1.0
    assert torch.equal(pcm, K.summary_audio_s16(out, count=3)) and np.array_equal(pcm.cpu().numpy(), RR.pcm16(on))
    # without normalisation the PCM clips, by the same rule
    plain, pcm, _ = K.resample(dev, *pair, normalize=False, want_pcm=True)
    assert torch.equal(plain, y) and np.array_equal(pcm.cpu().numpy(), RR.pcm16(yn)) and int(pcm[0].max()) == 32767
    # the entry point alone: no second launch is needed for y, and the peaks alone come without touching out
    code, raw, _, none = _raw(pair, dev, normalize=False, want_pcm=False, want_peak=False)
    assert code == 0 and none is None and torch.equal(raw, y)
    code, raw, _, only_peak = _raw(pair, dev, normalize=False, want_pcm=False, want_peak=True)
    assert code == 0 and torch.equal(raw, y) and torch.equal(only_peak, exact)
    code, raw, raw_pcm, none = _raw(pair, dev, normalize=True, want_pcm=True, want_peak=False)
    assert code == 0 and none is None and torch.equal(raw, out) and np.array_equal(raw_pcm.cpu().numpy(), RR.pcm16(on))


def test_two_calls_are_bit_identical():
    K = _K()
    x = (torch.rand(3, 5000, generator=torch.Generator().manual_seed(6)) * 4 - 2).cuda()
    for pair in [(16000, 44100), (48000, 16000)]:
        first = K.resample(x, *pair, normalize=True, want_pcm=True)
        second = K.resample(x, *pair, normalize=True, want_pcm=True)
        for a, b in zip(first, second):
            assert torch.equal(a, b)
    one = K.resample(x[1], 16000, 44100)[0]                  # a [n] input is a one-row batch, and a row does not depend on its neighbours
    assert one.shape[0] == 1 and torch.equal(one[0], K.resample(x, 16000, 44100)[0][1])


def test_the_design_is_cached_per_pair_and_device():
    K = _K()
    a = K.resample_design(16000, 48000, torch.device("cuda", torch.cuda.current_device()))
    b = K.resample_design(16000, 48000, "cuda")
    assert a[1] is b[1] and a[0] is b[0] and tuple(a[1].shape) == (3 * 68,)
    assert tuple(K.resample_design(44100, 16000, "cuda")[1].shape) == (160 * 188,)       # rows padded to 16 bytes


def test_public_resample():
    from gansynth_amd import spectral_ops
    x = (torch.rand(2, 3000, generator=torch.Generator().manual_seed(8)) * 2 - 1).cuda()
    assert spectral_ops.resample(x, 16000, 16000) is x
    up = spectral_ops.resample(x, 16000, 22050)
    assert tuple(up.shape) == (2, RR.out_len(3000, 441, 320)) and torch.equal(up, _K().resample(x, 16000, 22050)[0])
    _check(up.cpu().numpy(), x.cpu().numpy(), (16000, 22050), "spectral_ops.resample")
    assert tuple(spectral_ops.resample(x[0], 44100, 16000).shape) == (RR.out_len(3000, 160, 441),)
    with pytest.raises(Exception, match="up ="):
        spectral_ops.resample(x, 16000, 44101)


# ---------------------------------------------------------------------------------------------------------- end to end
KW = dict(batch_size=4, release_seconds=0.01, seconds_per_instrument=0.04, seed=2)


def test_synthesize_at_another_rate(gpu_store):
    from tests.test_notes_gpu import _model, _score
    K = _K()
    model, score = _model(), _score()
    mix = model.synthesize(score, normalize=False, **KW)                          # the unnormalised 16 kHz mix
    info16 = {}
    today = model.synthesize(score, want_pcm=True, info=info16, **KW)
    for rate in (None, 16000):                                                    # the model's own rate: today's path, bit for bit
        same = model.synthesize(score, want_pcm=True, sample_rate=rate, **KW)
        assert torch.equal(same[0], today[0]) and torch.equal(same[1], today[1])
    total = mix.numel()
    assert info16["sample_rate"] == 16000 and info16["output_samples"] == info16["total_samples"] == total
    info = {}
    clip, pcm = model.synthesize(score, want_pcm=True, sample_rate=48000, info=info, **KW)
    assert clip.dtype == torch.float32 and pcm.dtype == torch.int16 and tuple(clip.shape) == tuple(pcm.shape) == (3 * total,)
    assert (info["sample_rate"], info["output_samples"], info["total_samples"]) == (48000, 3 * total, total) and info["notes"] == info16["notes"]
    raw, _, peak = K.resample(mix, 16000, 48000)
    _check(raw.cpu().numpy(), mix.cpu().numpy(), (16000, 48000), "synthesize at 48 kHz")
    assert info["peak"] == float(peak[0]) == float(raw.abs().max())
    rn = raw[0].cpu().numpy()
    want = rn / np.float32(info["peak"]) if info["peak"] > 1.0 else rn             # the tail rule
    assert np.array_equal(clip.cpu().numpy(), want) and np.array_equal(pcm.cpu().numpy(), RR.pcm16(want))
    print(f"peak at 16 kHz {info16['peak']:.4f}, at 48 kHz {info['peak']:.4f}")
    plain = model.synthesize(score, normalize=False, sample_rate=48000, **KW)
    assert torch.equal(plain, raw[0])


def test_generate_at_another_rate(gpu_store):
    from gansynth_amd import spectral_ops
    from tests.test_model_gpu import cuda
    from tests.test_notes_gpu import _model
    model = _model()
    lat, lab, _ = R.synthetic_batch(4, rank=0)
    lat, lab = cuda(lat), cuda(lab)
    base = model.generate(lat, lab)
    assert torch.equal(model.generate(lat, lab, sample_rate=16000), base) and torch.equal(model.generate(lat, lab, sample_rate=None), base)
    got = model.generate(lat, lab, sample_rate=44100)
    assert tuple(got.shape) == (4, -(-1024 * 441 // 160)) == (4, 2823)
    assert torch.equal(got, spectral_ops.resample(base, 16000, 44100))            # row by row, not normalised
    _check(got.cpu().numpy(), base.cpu().numpy(), (16000, 44100), "generate at 44.1 kHz")


def test_driver_writes_the_new_rate(gpu_store, tmp_path):
    """What `gan_synth_main.py --synthesize score.json --output x.wav --output_rate 48000` runs after building its model."""
    from scipy.io import wavfile
    import gan_synth_main as main
    from tests import synth_ref as SRF
    from tests.test_notes_gpu import _model, _score
    model, score = _model(), _score()
    items = [dict(pitch=n.pitch, velocity=n.velocity, start=n.start, end=n.end) for n in score]
    (tmp_path / "score.json").write_text(json.dumps(items))
    args = main.parser.parse_args(["--synthesize", str(tmp_path / "score.json"), "--output", str(tmp_path / "x.wav"), "--batch_size", "4",
                                   "--release_seconds", "0.01", "--model_dir", str(tmp_path / "no_model"), "--output_rate", "48000"])
    lines = []
    info = main.synthesize_to_wav(model, args, range(24, 85), log=lines.append)
    rate, data = wavfile.read(str(tmp_path / "x.wav"))
    _, total, _, _ = SRF.schedule([tuple(n) for n in score], range(24, 85), 16000, 1024, 0.01)
    assert rate == 48000 and data.dtype == np.int16 and data.shape == (3 * total,)
    assert (info["sample_rate"], info["output_samples"], info["total_samples"]) == (48000, 3 * total, total)
    _, pcm = model.synthesize(score, want_pcm=True, batch_size=4, release_seconds=0.01, sample_rate=48000)
    assert np.array_equal(data, pcm.cpu().numpy()) and np.abs(data).max() > 0
    assert f"{total / 16000:.3f} seconds" in lines[-1] and "at 48000 Hz" in lines[-1]
