"""GPU: gs_note_mix against the float64 restatement of tests/synth_ref.py -- every sample within the derived bound
(M + 6) * 2^-24 * A, bit-exact where the arithmetic is exact -- bad tables that must not fault, peak / normalisation / PCM, and
GANSynth.synthesize end to end on the reduced PGGAN of tests/test_model_gpu.py::test_generate_vs_oracle.

The driver: `gan_synth_main.py --synthesize` as a fresh child process with the full-size generator takes about three seconds in all
(test_driver_writes_the_wav); the code the flag runs, gan_synth_main.synthesize_to_wav, is also called on the reduced model
(test_driver_path_with_the_reduced_model), and tests/test_notes_cpu.py::test_driver_flags checks the flags."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import torch_ref as R
from tests import stereo_ref as STR
from tests import synth_ref as SRF

pytestmark = pytest.mark.gpu
L = SRF.L
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _K():
    from gansynth_amd import kernels
    return kernels.get()


def _raw_mix(waves, table, total, normalize=False, want_pcm=False, want_peak=True, prefill=float("nan")):
    """gs_note_mix itself on `table` AS GIVEN (no validation, no sorting): (return code, out, pcm, peak)."""
    from gansynth_amd import _lib, kernels
    K = _K()
    arr = (_lib.GsMixNote * len(table))(*[_lib.GsMixNote(int(o), int(h), int(r), int(row), float(g)) for o, h, r, row, g in table])
    notes = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    out = torch.full((total,), prefill, dtype=torch.float32, device="cuda")
    pcm = torch.full((total,), 77, dtype=torch.int16, device="cuda") if want_pcm else None
    peak = torch.full((1,), -1.0, dtype=torch.float32, device="cuda") if want_peak else None
    ws = torch.empty(max(K.lib.gs_note_mix_workspace_bytes(total), 256), dtype=torch.uint8, device="cuda")
    code = K.lib.gs_note_mix(waves.data_ptr(), waves.shape[0], waves.shape[1], waves.stride(0), notes.data_ptr(), len(table), total,
                             1 if normalize else 0, out.data_ptr(), None if pcm is None else pcm.data_ptr(),
                             None if peak is None else peak.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream())
    torch.cuda.synchronize()
    return code, out, pcm, peak


def _check(got, waves, table, total, what):
    """Every sample within the bound of the float64 mix (uncovered samples: exactly 0); where one note alone sounds at full level with a
    gain of 1 the sample is the wave's own, bit for bit.  Returns the worst error / bound."""
    got = got.cpu().numpy()
    waves = waves.cpu().numpy()
    assert got.shape == (total,) and got.dtype == np.float32
    ref, a, m = SRF.mix(waves, table, total)
    err = np.abs(got.astype(np.float64) - ref)
    bound = SRF.bound(a, m)
    bad = np.flatnonzero(~(err <= bound))          # (NaN fails)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), got[bad[:4]].tolist(), ref[bad[:4]].tolist(), m[bad[:4]].tolist())
    alone = np.zeros(total, dtype=bool)
    own = np.zeros(total, dtype=np.float32)
    for onset, hold, release, row, gain in table:
        n = min(hold, total - onset)
        if gain == 1.0 and n > 0:
            alone[onset:onset + n] = True
            own[onset:onset + n] = waves[row, :n]
    alone &= m == 1
    assert np.array_equal(got[alone], own[alone]), what
    covered = a > 0
    worst = float((err[covered] / bound[covered]).max()) if covered.any() else 0.0
    print(f"{what}: worst error / bound = {worst:.3f}, up to {int(m.max())} notes on a sample, {int((m == 0).sum())} silent samples")
    return worst


@pytest.fixture(scope="module")
def dense():
    """The dense random case, its float64 mix and the kernel's unnormalised result, computed once."""
    waves, notes = SRF.dense_case()
    table, total, _, _ = SRF.schedule(notes, range(24, 85), SRF.SR, L, SRF.RELEASE / SRF.SR)
    dev = torch.from_numpy(waves).cuda()
    mix, _, peak = _K().note_mix(dev, table, total, normalize=False)
    return dict(waves=dev, table=table, total=total, mix=mix, peak=peak)


def test_mix_against_the_reference(dense):
    _check(dense["mix"], dense["waves"], dense["table"], dense["total"], "dense case")


SMALL = [(0, 900, 103, 0, 1.0), (3, 500, 0, 1, 0.5), (250, 64, 64, 2, 0.875), (990, 1, 400, 3, 0.7)]   # the last one cut at total = 1003


def test_the_mix_is_the_stated_fp32_sum(dense):
    """Bit for bit tests/synth_ref.py's mix_f32 -- fl(1 / (release + 1)), the envelope's product, gain * env, the product with the sample,
    the running sum in table order, every operation rounded on its own, none contracted -- on the dense case and on less than a tile
    with a 3-sample tail: the kernel's arithmetic is held to the header's words, not to a bound around them."""
    waves, table, total = dense["waves"], dense["table"], dense["total"]
    assert np.array_equal(dense["mix"].cpu().numpy(), SRF.mix_f32(waves.cpu().numpy(), table, total))
    few = STR.dense_table()[0][:4, :L]                                                  # (the waves of tests/test_ensemble_gpu.py's like-named case)
    out, _, _ = _K().note_mix(torch.from_numpy(few).cuda(), SMALL, 1003, normalize=False)
    assert np.array_equal(out.cpu().numpy(), SRF.mix_f32(few, SMALL, 1003))


def _waves(rows, length=L, seed=1):
    return (torch.rand(rows, length, generator=torch.Generator().manual_seed(seed)) * 2 - 1).cuda()


def test_a_single_full_note_is_its_wave():
    waves = _waves(3)
    out, _, peak = _K().note_mix(waves, [(0, L, 0, 1, 1.0)], L, normalize=False)
    assert torch.equal(out, waves[1]) and torch.equal(peak, waves[1].abs().max()[None])


def test_a_gap_between_notes_is_silence():
    from gansynth_amd import _lib
    tile = _lib.MIX_TILE
    waves = _waves(2)
    table = [(0, 100, 50, 0, 1.0), (3 * tile + 17, 200, 0, 1, 0.5)]      # more than two whole tiles no note covers
    total = 3 * tile + 217
    code, out, _, _ = _raw_mix(waves, table, total)                       # (out arrives full of NaN)
    assert code == 0
    assert torch.equal(out[150:3 * tile + 17], torch.zeros(3 * tile + 17 - 150, device="cuda"))
    _check(out, waves, table, total, "gap")


def test_placements():
    from gansynth_amd import _lib
    tile = _lib.MIX_TILE
    waves = _waves(6)
    table = [(tile - L, L, 0, 0, 1.0),                  # ends exactly on a tile edge
             (tile, 512, 512, 1, 0.75),                 # starts exactly on one
             (2 * tile - 300, 600, 100, 2, 1.0),        # crosses an edge
             (100, 1, 0, 3, 1.0), (205, 1, 7, 3, 0.3),  # hold = 1, with and without a release; the same row twice
             (301, 40, 9, 4, 1.0), (402, 40, 9, 4, 1.0), (503, 40, 9, 4, 1.0), (604, 40, 9, 4, 1.0),   # every residue mod 4
             (610, 30, 30, 5, 0.6)]
    total = 2 * tile + 400
    out, _, _ = _K().note_mix(waves, table, total, normalize=False)
    _check(out, waves, table, total, "placements")
    long = _waves(2, 3 * _lib.MIX_TILE, seed=2)         # a note that crosses three tile edges, another inside it
    table = [(tile - 5, 2 * tile + 100, 900, 0, 1.0), (2 * tile, 10, 10, 1, 0.5)]
    total = 3 * tile + 995
    out, _, _ = _K().note_mix(long, table, total, normalize=False)
    _check(out, long, table, total, "three tiles")


def test_two_notes_with_the_same_onset_in_both_orders():
    waves = _waves(2)
    a, b = (64, 300, 40, 0, 0.8), (64, 200, 100, 1, 0.35)
    first, _, _ = _K().note_mix(waves, [a, b], 500, normalize=False)
    second, _, _ = _K().note_mix(waves, [b, a], 500, normalize=False)
    _check(first, waves, [a, b], 500, "same onset")
    _check(second, waves, [b, a], 500, "same onset, exchanged")
    assert torch.equal(first, second)                   # a sum of two terms does not depend on their order


def test_short_clips_and_clipping_at_total():
    waves = _waves(2)
    table = [(0, 900, 103, 0, 1.0), (3, 500, 0, 1, 0.5)]
    out, pcm, _ = _K().note_mix(waves, table, 1003, normalize=False, want_pcm=True)     # 4 k + 3, smaller than a tile
    _check(out, waves, table, 1003, "total = 1003")
    assert np.array_equal(pcm.cpu().numpy(), SRF.pcm16(out.cpu().numpy()))
    for total in (7, 1, 4099):                                                         # notes that run past the end are cut there
        table = [(0, 1000, 24, 0, 1.0), (total - 1, 500, 100, 1, 0.5)]
        code, out, _, _ = _raw_mix(torch.cat([waves, waves]), table + [(total + 5, 10, 0, 2, 1.0)], total)   # (and one wholly beyond it)
        assert code == 0
        _check(out, waves, table, total, f"total = {total}")


def test_full_length_notes():
    """L = 64000: 8 notes over 2.5 s, several tiles per note."""
    length = 64000
    waves = _waves(8, length, seed=3)
    rng = np.random.default_rng(5)
    notes = [(int(rng.integers(24, 85)), int(rng.integers(1, 128)), float(s), float(s + d))
             for s, d in zip(rng.random(8) * 2.5, np.exp(rng.uniform(np.log(0.05), np.log(6.0), 8)))]
    table, total, _, _ = SRF.schedule(notes, range(24, 85), 16000, length, 1.0)
    assert any(h == length for _, h, _, _, _ in table) and any(0 < r < 16000 for _, _, r, _, _ in table)
    out, _, _ = _K().note_mix(waves, table, total, normalize=False)
    _check(out, waves, table, total, "L = 64000")


# name -> (the fields of the bad note, the field kernels.note_mix names)
BAD = {"row past the end": (dict(row=4), "row"), "negative row": (dict(row=-1), "row"), "huge row": (dict(row=2 ** 31 - 1), "row"),
       "hold 0": (dict(hold=0), "hold"), "negative hold": (dict(hold=-7), "hold"), "negative release": (dict(release=-1), "release"),
       "hold + release past L": (dict(hold=L, release=1), "release"),
       "hold + release past int32": (dict(hold=2 ** 31 - 1, release=2 ** 31 - 1), "hold"),
       "negative onset": (dict(onset=-5), "onset"), "onset at the far negative end": (dict(onset=-2 ** 63), "onset")}


@pytest.mark.parametrize("name", sorted(BAD))
def test_a_bad_note_is_skipped_not_followed(name):
    """One invalid field on one note of a valid table, handed to the entry point itself: the kernel validates every note before it touches
    memory, so the call succeeds and the result is the mix of the other notes, bit for bit.  (Nothing here can fault: that is the point.)"""
    waves = _waves(4)
    good = [(10, 400, 100, 0, 0.9), (300, L, 0, 1, 0.7), (350, 20, 160, 2, 1.0), (900, 700, 160, 3, 0.4), (1500, 64, 64, 0, 0.2)]
    total = 1700
    bad = dict(zip(("onset", "hold", "release", "row", "gain"), (340, 500, 160, 2, 0.8)), **BAD[name][0])
    table = sorted(good + [tuple(bad.values())], key=lambda n: n[0])               # (still sorted by onset)
    code, out, _, peak = _raw_mix(waves, table, total)
    assert code == 0
    code, want, _, want_peak = _raw_mix(waves, good, total)
    assert code == 0 and torch.equal(out, want) and torch.equal(peak, want_peak)
    _check(out, waves, good, total, name)
    with pytest.raises(ValueError, match=rf"field '{BAD[name][1]}'"):
        _K().note_mix(waves, table, total)


def test_peak_normalisation_and_pcm(dense):
    K = _K()
    mix, waves, table, total = dense["mix"], dense["waves"], dense["table"], dense["total"]
    exact_peak = mix.abs().max()
    assert float(exact_peak) > 1.0 and torch.equal(dense["peak"][0], exact_peak)
    out, pcm, peak = K.note_mix(waves, table, total, normalize=True, want_pcm=True)
    assert torch.equal(peak[0], exact_peak)                                         # a maximum is exact
    quotient = mix.cpu().numpy().astype(np.float64) / float(exact_peak)
    got = out.cpu().numpy()
    assert (np.abs(got.astype(np.float64) - quotient) <= np.spacing(np.abs(quotient).astype(np.float32))).all()     # 1 ulp
    assert float(out.abs().max()) == 1.0
    assert torch.equal(pcm, K.summary_audio_s16(out[None])[0]) and np.array_equal(pcm.cpu().numpy(), SRF.pcm16(got))
    # determinism: a second call, bit for bit
    again, pcm2, peak2 = K.note_mix(waves, table, total, normalize=True, want_pcm=True)
    assert torch.equal(again, out) and torch.equal(pcm2, pcm) and torch.equal(peak2, peak)
    # without normalisation the PCM clips, by the same rule
    plain, pcm, _ = K.note_mix(waves, table, total, normalize=False, want_pcm=True)
    assert torch.equal(plain, mix) and torch.equal(pcm, K.summary_audio_s16(mix[None])[0])
    # a quiet clip is left alone
    quiet = waves * 0.03125
    want, _, _ = K.note_mix(quiet, table, total, normalize=False)
    out, pcm, peak = K.note_mix(quiet, table, total, normalize=True, want_pcm=True)
    assert float(peak) <= 1.0 and torch.equal(peak[0], want.abs().max()) and torch.equal(out, want)
    assert torch.equal(pcm, K.summary_audio_s16(out[None])[0])
    # the entry point alone: no second launch is needed for the mix, and the peak alone comes without touching out
    code, raw, _, none = _raw_mix(waves, table, total, want_peak=False)
    assert code == 0 and none is None and torch.equal(raw, mix)
    code, raw, _, only_peak = _raw_mix(waves, table, total, want_peak=True)
    assert code == 0 and torch.equal(raw, mix) and torch.equal(only_peak[0], exact_peak)


# ---------------------------------------------------------------------------------------------------------- end to end
P = dict(waveform_length=1024, sample_rate=16000, spectrogram_shape=[16, 128], overlap=0.75)


def _model():
    """The reduced PGGAN and spectral parameters of tests/test_model_gpu.py::test_generate_vs_oracle, in the current default store."""
    from gansynth_amd.utils import Dict
    from tests.test_model_gpu import cuda, make
    pg, opg, model = make(1.0, None, full=False)
    lat, lab, _ = R.synthetic_batch(4, rank=0)
    gp, dp = opg.init_params(seed=3, bias_std=0.1)
    model._build(cuda(lat), cuda(lab))
    model.store.load_state_dict({**gp, **dp})
    model.spectral_params = Dict(P)
    return model


def _score():
    from gansynth_amd.notes import Note
    rng = np.random.default_rng(11)
    return [Note(int(p), int(v), float(s), float(s + d)) for p, v, s, d in
            zip(rng.integers(24, 85, 10), rng.integers(1, 128, 10), rng.random(10) * 0.15, np.exp(rng.uniform(np.log(0.002), np.log(0.1), 10)))]


def test_synthesize_end_to_end(gpu_store, tmp_path):
    from gansynth_amd import checkpoint
    from gansynth_amd.notes import Note
    model = _model()
    score = _score()
    g_before, d_before, step = model.g_params.flat.clone(), model.d_params.flat.clone(), model.global_step
    cpu_rng, gpu_rng = torch.random.get_rng_state(), torch.cuda.get_rng_state()
    info = {}
    clip = model.synthesize(score, normalize=False, info=info, batch_size=4, release_seconds=0.01, seconds_per_instrument=0.04, seed=2)
    assert torch.equal(torch.random.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
    assert torch.equal(model.g_params.flat, g_before) and torch.equal(model.d_params.flat, d_before) and model.global_step == step
    table, total, kept, dropped = SRF.schedule([tuple(n) for n in score], range(24, 85), 16000, 1024, 0.01)
    assert info["dropped"] == dropped == 0 and info["total_samples"] == total == clip.numel() and info["notes"] == [score[i] for i in kept]
    assert tuple(info["latents"].shape) == (10, 256) and info["latents"].dtype == torch.float32
    assert clip.dtype == torch.float32 and clip.is_cuda and info["peak"] == float(clip.abs().max())
    anchors = torch.randn(math.floor(total / 16000 / 0.04) + 2, 256, generator=torch.Generator().manual_seed(2)).double().numpy()
    assert np.abs(info["latents"].numpy() - SRF.note_latents(anchors, [n.start for n in info["notes"]], 0.04)).max() <= 1e-6
    # the waves of the same padded chunks, through model.generate
    labels = torch.eye(61)[[n.pitch - 24 for n in info["notes"]]]
    waves = torch.empty(10, 1024, device="cuda")
    for lo in (0, 4, 8):
        rows = [min(i, 9) for i in range(lo, lo + 4)]
        waves[lo:lo + 4] = model.generate(info["latents"][rows].cuda(), labels[rows].cuda())[:min(4, 10 - lo)]
    _check(clip, waves, table, total, "synthesize")
    # one note at full velocity and full length is that note's waveform
    one = [Note(60, 127, 0.0, 0.5)]
    solo_info = {}
    solo = model.synthesize(one, normalize=False, info=solo_info, batch_size=4, latents=info["latents"][3])
    want = model.generate(info["latents"][3][None].expand(4, -1).cuda(), torch.eye(61)[[36] * 4].cuda())[0]
    assert solo.numel() == 1024 and torch.equal(solo, want) and torch.equal(solo_info["latents"][0], info["latents"][3])
    # model_dir: the latest checkpoint is restored first, as generate does
    checkpoint.save(model, str(tmp_path))
    for p in model.g_params.named.values():
        p.data.add_(0.125)
    assert not torch.equal(model.g_params.flat, g_before)
    restored_clip = model.synthesize(score, model_dir=str(tmp_path), normalize=False, batch_size=4, release_seconds=0.01,
                                    seconds_per_instrument=0.04, seed=2)
    assert torch.equal(model.g_params.flat, g_before) and torch.equal(restored_clip, clip)


def test_a_train_step_after_synthesize_is_the_same_step():
    from gansynth_amd import variables
    from tests.test_model_gpu import cuda
    old = variables._default
    losses = []
    try:
        for with_synthesize in (False, True):
            variables.set_default_store(variables.VariableStore(device="cuda"))
            torch.manual_seed(17)
            model = _model()
            if with_synthesize:
                model.synthesize(_score(), batch_size=4, release_seconds=0.01)
            lat, lab, real = R.synthetic_batch(4, rank=1, image_shape=(2, 16, 128))
            d = torch.as_tensor(model.discriminator_step(cuda(lat), cuda(lab), cuda(real))).detach().clone()
            g = torch.as_tensor(model.generator_step(cuda(lat), cuda(lab))).detach().clone()
            losses.append((d, g, model.g_params.flat.clone(), model.d_params.flat.clone()))
    finally:
        variables._default = old
    for a, b in zip(*losses):
        assert torch.equal(a, b)


def test_driver_path_with_the_reduced_model(gpu_store, tmp_path):
    """What `gan_synth_main.py --synthesize score.json --output x.wav` runs after building its model."""
    from scipy.io import wavfile
    import gan_synth_main as main
    model = _model()
    score = _score()
    items = [dict(pitch=n.pitch, velocity=n.velocity, start=n.start, end=n.end) for n in score] + [dict(pitch=100, velocity=9, start=0.0, end=1.0)]
    (tmp_path / "score.json").write_text(json.dumps(items))
    args = main.parser.parse_args(["--synthesize", str(tmp_path / "score.json"), "--output", str(tmp_path / "x.wav"), "--batch_size", "4",
                                   "--release_seconds", "0.01", "--model_dir", str(tmp_path / "no_model")])
    lines = []
    info = main.synthesize_to_wav(model, args, range(24, 85), log=lines.append)
    rate, data = wavfile.read(str(tmp_path / "x.wav"))
    _, total, _, _ = SRF.schedule([tuple(n) for n in score], range(24, 85), 16000, 1024, 0.01)
    assert rate == 16000 and data.dtype == np.int16 and data.shape == (total,) and info["total_samples"] == total
    _, pcm = model.synthesize(score, want_pcm=True, batch_size=4, release_seconds=0.01)
    assert np.array_equal(data, pcm.cpu().numpy()) and np.abs(data).max() > 0
    assert "no checkpoint found" in lines[0] and "10 notes kept, 1 dropped" in lines[-1] and f"{total / 16000:.3f} seconds" in lines[-1]


def test_driver_writes_the_wav(tmp_path):
    """`gan_synth_main.py --synthesize score.json --output x.wav` in a fresh process: no dataset, no checkpoint (the initial weights), the
    full-size generator, a short score."""
    from scipy.io import wavfile
    items = [dict(pitch=60 + i, velocity=100, start=0.25 * i, end=0.25 * i + 0.5) for i in range(4)] + [dict(pitch=10, velocity=1, start=0.0, end=9.0)]
    (tmp_path / "score.json").write_text(json.dumps(items))
    cmd = [sys.executable, os.path.join(ROOT, "gan_synth_main.py"), "--synthesize", str(tmp_path / "score.json"), "--output", str(tmp_path / "x.wav"),
           "--model_dir", str(tmp_path / "model"), "--release_seconds", "0.5"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    _, total, _, dropped = SRF.schedule([(n["pitch"], n["velocity"], n["start"], n["end"]) for n in items], range(24, 85), 16000, 64000, 0.5)
    assert total == 12000 + 8000 + 8000 and dropped == 1
    rate, data = wavfile.read(str(tmp_path / "x.wav"))
    assert rate == 16000 and data.dtype == np.int16 and data.shape == (total,) and np.abs(data.astype(np.int32)).max() > 0
    assert "no checkpoint found" in r.stdout and f"4 notes kept, 1 dropped, {total / 16000:.3f} seconds, peak " in r.stdout

