"""GPU: gs_note_mix_stereo against gs_note_mix (each channel bit for bit the mono mix with that channel's gain) and against the float64
restatement of tests/stereo_ref.py within tests/synth_ref.py's own bound (M + 6) * 2^-24 * A; the joint peak, the quotient and the
interleaved PCM; both store paths; bad tables that must be skipped; gs_stereo_finish on clips of its own; and
GANSynth.synthesize(ensemble=True, stereo=True) end to end on the reduced PGGAN of tests/test_notes_gpu.py, at the model's rate and at 24 kHz.
tests/test_ensemble_cpu.py::test_fp32_evaluation_sits_inside_the_bound shows on the CPU that an honest fp32 evaluation of the tables used
here sits inside that bound."""
import json

import numpy as np
import pytest
import torch

from tests import stereo_ref as STR
from tests import synth_ref as SRF

pytestmark = pytest.mark.gpu
L, TOTAL = STR.LENGTH, STR.TOTAL
SENTINEL, PCM_SENTINEL, PAD = 12345.0, 77, 64


def _K():
    from gansynth_amd import kernels
    return kernels.get()


def _raw(waves, table, total, normalize=False, want_pcm=False, want_peak=True, offset=0, stride=None):
    """gs_note_mix_stereo itself on `table` AS GIVEN (no validation, no sorting), `out` and `pcm` inside buffers full of a sentinel:
    -> (out [2, total], pcm [total, 2] or None, peak or None) after checking that the call succeeded and that nothing but the two rows'
    [0, total) and the PCM's [0, 2 total) was written.  `offset`: floats by which the base of out is moved off its 16-byte alignment."""
    from gansynth_amd import _lib, kernels
    K = _K()
    stride = (total + 3) // 4 * 4 if stride is None else stride
    arr = (_lib.GsMixNoteStereo * len(table))(*[_lib.GsMixNoteStereo(int(o), int(h), int(r), int(row), float(gl), float(gr), 0) for o, h, r, row, gl, gr in table])
    notes = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    buf = torch.full((PAD + offset + 2 * stride + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[PAD + offset:PAD + offset + 2 * stride].view(2, stride)
    pbuf = torch.full((PAD + 2 * total + PAD,), PCM_SENTINEL, dtype=torch.int16, device="cuda") if want_pcm else None
    pcm = pbuf[PAD:PAD + 2 * total].view(total, 2) if want_pcm else None
    peak = torch.full((1,), -1.0, dtype=torch.float32, device="cuda") if want_peak else None
    ws = torch.empty(max(K.lib.gs_note_mix_stereo_workspace_bytes(total), 256), dtype=torch.uint8, device="cuda")
    code = K.lib.gs_note_mix_stereo(waves.data_ptr(), waves.shape[0], waves.shape[1], waves.stride(0), notes.data_ptr(), len(table), total,
                                    1 if normalize else 0, out.data_ptr(), stride, None if pcm is None else pcm.data_ptr(),
                                    None if peak is None else peak.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream())
    torch.cuda.synchronize()
    assert code == 0, K.lib.gs_last_error()
    assert (buf[:PAD + offset] == SENTINEL).all() and (buf[PAD + offset + 2 * stride:] == SENTINEL).all() and (out[:, total:] == SENTINEL).all()
    if want_pcm:
        assert (pbuf[:PAD] == PCM_SENTINEL).all() and (pbuf[PAD + 2 * total:] == PCM_SENTINEL).all()
    return out[:, :total], pcm, peak


def _mono(waves, table, total):
    """gs_note_mix's unnormalised mix of each side: ([left, right], [peak_l, peak_r])."""
    got = [_K().note_mix(waves, STR.side(table, c), total, normalize=False) for c in (0, 1)]
    return [g[0] for g in got], [g[2] for g in got]


@pytest.fixture(scope="module")
def dense():
    """The dense tables (the louder side left, then right), their waves as rows 1100 apart and the kernel's unnormalised mixes: once."""
    cases = {}
    for lean in (0.2, 0.8):
        waves, table = STR.dense_table(lean=lean)
        dev = torch.from_numpy(waves).cuda()[:, :L]                      # [40, 1024], row stride 1100
        assert dev.stride(0) == STR.STRIDE
        mix, _, peak = _raw(dev, table, TOTAL)
        cases[lean] = dict(host=waves[:, :L], waves=dev, table=table, mix=mix.clone(), peak=peak)
    return cases


SMALL = [(0, 900, 103, 0, 1.0, 0.25), (3, 500, 0, 1, 0.5, 0.5), (250, 64, 64, 2, 0.0, 0.875), (990, 1, 400, 3, 0.7, 0.1)]   # the last one cut at total


@pytest.mark.parametrize("case", ["three tiles", "less than a tile", "one note"])
def test_each_channel_is_the_mono_mix(dense, case):
    if case == "three tiles":
        waves, table, total, got = dense[0.2]["waves"], dense[0.2]["table"], TOTAL, dense[0.2]["mix"]
        peak = dense[0.2]["peak"]
    else:
        waves = dense[0.2]["waves"]
        table, total = (SMALL, 1003) if case == "less than a tile" else ([(5, 300, 200, 7, 0.8, 0.3)], 505)
        got, _, peak = _raw(waves, table, total)
    (left, right), (peak_l, peak_r) = _mono(waves, table, total)
    assert got.shape == (2, total) and torch.equal(got[0], left) and torch.equal(got[1], right)
    assert torch.equal(peak, torch.maximum(peak_l, peak_r))
    only_mix, _, none = _raw(waves, table, total, want_peak=False)          # the first launch alone
    assert none is None and torch.equal(only_mix, got)


def test_each_side_is_the_stated_fp32_sum(dense):
    """Bit for bit tests/stereo_ref.py's mix_f32 -- tests/synth_ref.py's fp32 sum in the stated order, side by side -- on three tiles and
    on less than a tile with a 3-sample tail: both channels of the one kernel are held to the header's words themselves."""
    d = dense[0.2]
    assert np.array_equal(d["mix"].cpu().numpy(), STR.mix_f32(d["host"], d["table"], TOTAL))
    got, _, _ = _raw(d["waves"], SMALL, 1003)
    assert np.array_equal(got.cpu().numpy(), STR.mix_f32(d["host"], SMALL, 1003))


@pytest.mark.parametrize("lean", [0.2, 0.8])
def test_mix_against_the_reference(dense, lean):
    d = dense[lean]
    ref, a, m = STR.mix(d["host"], d["table"], TOTAL)
    got = d["mix"].cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref)
    bound = SRF.bound(a, m[None])
    bad = np.argwhere(~(err <= bound))                                     # (NaN fails)
    assert bad.size == 0, (len(bad), bad[:4].tolist())
    assert (got[a == 0] == 0).all()                                        # no note: exactly 0, on a buffer that arrived full of a sentinel
    print(f"lean {lean}: worst error / bound = {(err[a > 0] / bound[a > 0]).max():.3f}, up to {int(m.max())} notes on a sample")


@pytest.mark.parametrize("lean", [0.2, 0.8])
def test_joint_peak_quotient_and_pcm(dense, lean):
    d = dense[lean]
    waves, table, mix = d["waves"], d["table"], d["mix"]
    _, (peak_l, peak_r) = _mono(waves, table, TOTAL)
    assert float(peak_l) > 1.0 and float(peak_r) > 1.0 and (float(peak_r) > float(peak_l)) == (lean > 0.5)
    out, pcm, peak = _raw(waves, table, TOTAL, normalize=True, want_pcm=True)
    assert torch.equal(peak, torch.maximum(peak_l, peak_r)) and torch.equal(peak, d["peak"])
    want_peak, want, want_pcm = STR.finish(mix.cpu().numpy(), True)
    assert float(peak) == float(want_peak)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(pcm.cpu().numpy(), want_pcm)
    assert float(out.abs().max()) == 1.0 and float(out[0 if lean > 0.5 else 1].abs().max()) < 1.0      # ONE peak: the quieter side stays quieter
    # without normalisation the mix is left alone and the PCM clips, by the same rule
    plain, pcm, _ = _raw(waves, table, TOTAL, normalize=False, want_pcm=True)
    assert torch.equal(plain, mix) and np.array_equal(pcm.cpu().numpy(), STR.finish(mix.cpu().numpy(), False)[2])
    # through the Python layer: the same three results
    out2, pcm2, peak2 = _K().note_mix_stereo(waves, table, TOTAL, normalize=True, want_pcm=True)
    assert out2.shape == (2, TOTAL) and out2.stride(0) % 4 == 0 and pcm2.shape == (TOTAL, 2) and pcm2.is_contiguous()
    assert torch.equal(out2, out) and np.array_equal(pcm2.cpu().numpy(), want_pcm) and torch.equal(peak2, peak)


def test_a_quiet_clip_is_left_alone(dense):
    d = dense[0.2]
    quiet = (d["waves"] * 0.03125).contiguous()
    want, _, _ = _raw(quiet, d["table"], TOTAL)
    out, pcm, peak = _raw(quiet, d["table"], TOTAL, normalize=True, want_pcm=True)
    assert 0.0 < float(peak) <= 1.0 and torch.equal(peak[0], want.abs().max()) and torch.equal(out, want)
    assert np.array_equal(pcm.cpu().numpy(), STR.finish(want.cpu().numpy(), True)[2])


def test_store_paths_and_determinism(dense):
    d = dense[0.8]
    waves, table = d["waves"], d["table"]
    out, pcm, peak = _raw(waves, table, TOTAL, normalize=True, want_pcm=True)
    again = _raw(waves, table, TOTAL, normalize=True, want_pcm=True)
    assert torch.equal(again[0], out) and torch.equal(again[1], pcm) and torch.equal(again[2], peak)
    off = _raw(waves, table, TOTAL, normalize=True, want_pcm=True, offset=1)                  # out off 16 bytes: sample by sample
    assert off[0].data_ptr() % 16 == 4 and out.data_ptr() % 16 == 0
    assert torch.equal(off[0], out) and torch.equal(off[1], pcm) and torch.equal(off[2], peak)
    odd = _raw(waves, table, TOTAL, normalize=True, want_pcm=True, stride=TOTAL + 1)          # row 1 alone off 16 bytes
    assert (TOTAL + 1) % 4 != 0 and torch.equal(odd[0], out) and torch.equal(odd[1], pcm) and torch.equal(odd[2], peak)
    unscaled = _raw(waves, table, TOTAL, offset=1)[0]
    assert torch.equal(unscaled, d["mix"])


# name -> the fields of the bad note
BAD = {"negative row": dict(row=-1), "row past the end": dict(row=4), "hold 0": dict(hold=0), "hold + release past L": dict(hold=L, release=1),
       "negative onset": dict(onset=-5)}


@pytest.mark.parametrize("name", sorted(BAD))
def test_a_bad_note_is_skipped_not_followed(name):
    """One invalid field on one note of a valid table, handed to the entry point itself: the kernel judges every note before it forms an
    address from it, so the call succeeds, the result is the mix of the other notes bit for bit, and nothing around out and pcm is
    written (_raw checks the sentinels).  Nothing here can fault: that is the point."""
    waves = (torch.rand(4, L, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    good = [(10, 400, 100, 0, 0.9, 0.2), (300, L, 0, 1, 0.7, 0.7), (350, 20, 160, 2, 1.0, 0.0), (900, 700, 160, 3, 0.4, 0.6), (1500, 64, 64, 0, 0.2, 0.9)]
    total = 1700
    bad = dict(zip(("onset", "hold", "release", "row", "gain_l", "gain_r"), (340, 500, 160, 2, 0.8, 0.8)), **BAD[name])
    table = sorted(good + [tuple(bad.values())], key=lambda n: n[0])                # (still sorted by onset)
    out, pcm, peak = _raw(waves, table, total, normalize=True, want_pcm=True)
    want, want_pcm, want_peak = _raw(waves, good, total, normalize=True, want_pcm=True)
    assert torch.equal(out, want) and torch.equal(pcm, want_pcm) and torch.equal(peak, want_peak)
    (left, right), _ = _mono(waves, good, total)
    assert torch.equal(_raw(waves, table, total)[0], torch.stack([left, right]))
    with pytest.raises(ValueError, match="note_mix_stereo: note "):
        _K().note_mix_stereo(waves, table, total)


@pytest.mark.parametrize("n,extra", [(9004, 0), (9004, 5), (9003, 0), (9003, 5)])
def test_stereo_finish(n, extra):
    """A [2, n] clip of its own, rows n + extra apart (n + 5: row 1 off 16 bytes, and a gap that must stay as it is)."""
    from gansynth_amd import kernels
    K = _K()
    stride = n + extra
    rng = np.random.default_rng(n + extra)
    host = np.clip(rng.standard_normal((2, n)) * 0.8, -3.0, 3.0).astype(np.float32)
    host[1, n - 2] = -3.25                                              # the peak: on the right, in the tail
    assert n % 4 in (0, 3) and np.abs(host).max() == 3.25

    def clip(values):
        buf = torch.full((PAD + 2 * stride + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        x = buf[PAD:PAD + 2 * stride].view(2, stride)[:, :n]
        x.copy_(torch.from_numpy(values))
        return buf, x

    def untouched(buf):
        return bool((buf[:PAD] == SENTINEL).all() and (buf[PAD + 2 * stride:] == SENTINEL).all() and
                    (buf[PAD:PAD + 2 * stride].view(2, stride)[:, n:] == SENTINEL).all())

    want_peak, want, want_pcm = STR.finish(host, True)
    buf, x = clip(host)
    got, pcm, peak = K.stereo_finish(x, normalize=True, want_pcm=True)
    assert got.data_ptr() == x.data_ptr() and float(peak) == float(want_peak) == 3.25 and untouched(buf)
    assert np.array_equal(x.cpu().numpy(), want) and pcm.shape == (n, 2) and np.array_equal(pcm.cpu().numpy(), want_pcm)
    # normalize = 0, no PCM: x is only read
    buf, x = clip(host)
    _, none, peak = K.stereo_finish(x, normalize=False, want_pcm=False)
    assert none is None and float(peak) == 3.25 and np.array_equal(x.cpu().numpy(), host) and untouched(buf)
    # normalize = 0 with PCM: x as it is, the PCM clipped
    _, pcm, _ = K.stereo_finish(x, normalize=False, want_pcm=True)
    assert np.array_equal(x.cpu().numpy(), host) and np.array_equal(pcm.cpu().numpy(), STR.finish(host, False)[2])
    # a quiet clip is left alone, its PCM taken
    buf, x = clip(host * np.float32(0.25))
    _, pcm, peak = K.stereo_finish(x, normalize=True, want_pcm=True)
    assert float(peak) == 0.8125 and np.array_equal(x.cpu().numpy(), host * np.float32(0.25)) and untouched(buf)
    assert np.array_equal(pcm.cpu().numpy(), STR.finish(host * np.float32(0.25), True)[2])
    # the entry point with a PCM base off 16 bytes: the sample-by-sample path, the same numbers
    buf, x = clip(host)
    pbuf = torch.full((PAD + 1 + 2 * n + PAD,), PCM_SENTINEL, dtype=torch.int16, device="cuda")
    peak = torch.zeros(1, device="cuda")
    ws = torch.empty(max(K.lib.gs_stereo_finish_workspace_bytes(n), 256), dtype=torch.uint8, device="cuda")
    code = K.lib.gs_stereo_finish(x.data_ptr(), n, stride, 1, pbuf[PAD + 1:].data_ptr(), peak.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream())
    torch.cuda.synchronize()
    assert code == 0 and float(peak) == 3.25 and np.array_equal(x.cpu().numpy(), want) and untouched(buf)
    assert np.array_equal(pbuf[PAD + 1:PAD + 1 + 2 * n].view(n, 2).cpu().numpy(), want_pcm)
    assert (pbuf[:PAD + 1] == PCM_SENTINEL).all() and (pbuf[PAD + 1 + 2 * n:] == PCM_SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------- end to end
def _parts_score():
    """The ten notes of tests/test_notes_gpu.py's score as JSON bytes in three parts: part 0 panned, parts 4 and 9 not; volumes that differ."""
    from tests.test_notes_gpu import _score
    items = []
    for i, n in enumerate(_score()):
        item = dict(pitch=n.pitch, velocity=n.velocity, start=n.start, end=n.end, part=(0, 4, 9)[i % 3], volume=(127, 100, 64)[i % 3])
        if i % 3 == 0:
            item["pan"] = (-0.5, 0.75)[(i // 3) % 2]
        items.append(item)
    items.append(dict(pitch=100, velocity=9, start=0.0, end=1.0, part=4))           # not in the label table: dropped
    return json.dumps(items).encode()


def _hand_waves(model, info, batch):
    """The notes' waves as synthesize generates them: chunks of `batch`, the last one padded by repeating its last row."""
    kept, lat = info["notes"], info["latents"]
    labels = torch.eye(61)[[n.pitch - 24 for n in kept]]
    waves = torch.empty(len(kept), 1024, device="cuda")
    for lo in range(0, len(kept), batch):
        rows = [min(i, len(kept) - 1) for i in range(lo, lo + batch)]
        waves[lo:lo + batch] = model._generate_batch(lat[rows].cuda(), labels[rows].cuda())[:min(batch, len(kept) - lo)]
    return waves


def test_synthesize_ensemble_stereo_end_to_end(gpu_store):
    from gansynth_amd import notes as N
    from tests.test_notes_gpu import _model
    K = _K()
    model = _model()
    data = _parts_score()
    score = N.read_score(data)
    kw = dict(batch_size=4, release_seconds=0.01, seconds_per_instrument=0.04, seed=2)
    before = model.synthesize(data, **kw)
    info = {}
    clip, pcm = model.synthesize(data, ensemble=True, stereo=True, spread=0.5, want_pcm=True, info=info, **kw)
    # the schedule, from the host functions
    index = N.kept_indices(score.notes, range(24, 85))
    kept, table, total, dropped = N.schedule(score.notes, range(24, 85), 16000, 1024, 0.01)
    assert info["notes"] == kept == [score.notes[i] for i in index] and info["dropped"] == dropped == 1 and info["total_samples"] == total
    assert info["parts"] == [N.Part(None, None)] * 3 and info["part_of_note"] == [score.part[i] for i in index] and info["channels"] == 2
    assert set(info["part_of_note"]) == {0, 1, 2}
    assert torch.equal(info["latents"], N.schedule_part_latents(kept, info["part_of_note"], 3, total, 16000, 2, 0.04))
    assert clip.shape == (2, total) and clip.dtype == torch.float32 and clip.is_cuda and pcm.shape == (total, 2) and pcm.dtype == torch.int16
    # the hand composition: the same waves, ONE stereo mix with schedule_gains' table
    waves = _hand_waves(model, info, 4)
    gains = N.schedule_gains(index, score, 0.5)
    assert {(l > r) - (l < r) for l, r in gains} == {1, -1}                          # notes left and right of the centre
    stereo_table = [row[:4] + g for row, g in zip(table, gains)]
    want, want_pcm, want_peak = K.note_mix_stereo(waves, stereo_table, total, normalize=True, want_pcm=True)
    assert torch.equal(clip, want) and torch.equal(pcm, want_pcm) and info["peak"] == float(want_peak)
    assert info["sample_rate"] == 16000 and info["output_samples"] == total
    # at 24 kHz: the unnormalised mix, one resample of its two rows, one finish there
    info24 = {}
    clip24, pcm24 = model.synthesize(data, ensemble=True, stereo=True, spread=0.5, want_pcm=True, info=info24, sample_rate=24000, **kw)
    mix, _, _ = K.note_mix_stereo(waves, stereo_table, total, normalize=False)
    up, _, _ = K.resample(mix, 16000, 24000, normalize=False)
    want, want_pcm, want_peak = K.stereo_finish(up, normalize=True, want_pcm=True)
    n24 = -(-total * 3 // 2)
    assert clip24.shape == (2, n24) and pcm24.shape == (n24, 2) and info24["output_samples"] == n24 and info24["sample_rate"] == 24000
    assert torch.equal(clip24, want) and torch.equal(pcm24, want_pcm) and info24["peak"] == float(want_peak) and info24["channels"] == 2
    # ensemble alone: mono through gs_note_mix, the volume in the gain
    mono_info = {}
    mono = model.synthesize(data, ensemble=True, info=mono_info, **kw)
    gain_table = [row[:4] + (score.notes[i].velocity * score.volume[i] / 127.0 ** 2,) for row, i in zip(table, index)]
    assert torch.equal(mono_info["latents"], info["latents"]) and mono_info["channels"] == 1
    assert torch.equal(mono, K.note_mix(waves, gain_table, total, normalize=True)[0])
    # stereo alone: one instrument (schedule_latents), no volume; a list of Note is one part in the centre: both channels the same
    solo_info = {}
    solo = model.synthesize(N.read_notes(data), stereo=True, spread=1.0, normalize=False, info=solo_info, **kw)
    assert torch.equal(solo_info["latents"], N.schedule_latents(kept, total, 16000, 2, 0.04)) and solo_info["parts"] == [N.Part(None, None)]
    assert solo.shape == (2, total) and torch.equal(solo[0], solo[1]) and float(solo.abs().max()) > 0
    with pytest.raises(ValueError, match="spread"):
        model.synthesize(data, stereo=True, spread=1.5, **kw)
    # the plain call is what it was
    after_info = {}
    after = model.synthesize(data, info=after_info, **kw)
    assert torch.equal(after, before) and after.shape == (total,) and "parts" not in after_info and "channels" not in after_info


def test_driver_writes_two_channels(gpu_store, tmp_path):
    """What `gan_synth_main.py --synthesize score.json --ensemble --stereo --spread 0.5` runs after building its model."""
    from scipy.io import wavfile
    import gan_synth_main as main
    from tests.test_notes_gpu import _model
    model = _model()
    (tmp_path / "score.json").write_bytes(_parts_score())
    args = main.parser.parse_args(["--synthesize", str(tmp_path / "score.json"), "--output", str(tmp_path / "x.wav"), "--batch_size", "4",
                                   "--release_seconds", "0.01", "--model_dir", str(tmp_path / "no_model"), "--ensemble", "--stereo", "--spread", "0.5"])
    lines = []
    info = main.synthesize_to_wav(model, args, range(24, 85), log=lines.append)
    rate, data = wavfile.read(str(tmp_path / "x.wav"))
    total = info["total_samples"]
    assert rate == 16000 and data.dtype == np.int16 and data.shape == (total, 2) and info["channels"] == 2
    _, pcm = model.synthesize(str(tmp_path / "score.json"), want_pcm=True, batch_size=4, release_seconds=0.01, ensemble=True, stereo=True, spread=0.5)
    assert np.array_equal(data, pcm.cpu().numpy()) and np.abs(data).max() > 0 and not np.array_equal(data[:, 0], data[:, 1])
    assert "10 notes kept, 1 dropped" in lines[-1]
