"""CPU: the event-file writer of gansynth_amd/summary.py (framing, checksums, protobuf, PNG, WAV), its host statement of the two
quantisation rules, and GANSynth.train with summaries on the CPU emulation backend.  Readers and references: tests/summary_ref.py."""
import glob
import os

import numpy as np
import torch

from tests import summary_ref as SR


def _events_files(model_dir):
    return sorted(glob.glob(os.path.join(str(model_dir), "events.out.tfevents.*")))


# -------------------------------------------------------------------------------------------------------------- checksum
def test_crc32c_known_answers():
    from gansynth_amd import summary
    for crc in (summary.crc32c, SR.crc32c):
        assert crc(b"123456789") == 0xE3069283
        assert crc(bytes(32)) == 0x8A9136AA
        assert crc(b"\xff" * 32) == 0x62A8AB43


def test_crc32c_of_a_long_message_equals_the_bitwise_form():
    """Long messages take the lane-parallel form (summary.crc32c): any length, any head."""
    from gansynth_amd import summary
    rng = np.random.default_rng(3)
    for n in (8 * 1024 - 1, 8 * 1024, 8 * 1024 + 1, 20011):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert summary.crc32c(data) == SR.crc32c(data), n


# ------------------------------------------------------------------------------------------------------------ round trip
def _inputs():
    g = torch.Generator().manual_seed(4)
    images = torch.randn(3, 2, 5, 37, generator=g)
    images[1, 1] = images[1, 1].abs()          # a plane of the other branch
    images[2, 0, 0, 0] = float("nan")
    audio = torch.from_numpy(SR.audio_case().copy())
    return images, audio


def test_round_trip(tmp_path):
    from gansynth_amd import summary
    images, audio = _inputs()
    with summary.SummaryWriter(str(tmp_path)) as w:
        w.scalars(7, dict(generator_loss=0.1, discriminator_loss=-2.5))
        w.images(8, {("mag", "freq"): images, "single": images[:, 0]})
        w.audio(9, dict(notes=audio), 16000)
        w.flush()
        path = w.path
    (found,) = _events_files(tmp_path)
    assert found == path
    name = os.path.basename(path).split(".")
    assert name[:3] == ["events", "out", "tfevents"] and len(name[3]) == 10 and name[3].isdigit() and len(name) >= 5
    assert SR.check_record_crcs(path) == 4
    events = SR.read_events(path)
    assert events[0]["file_version"] == "brain.Event:2" and events[0]["values"] == [] and events[0]["wall_time"] > 1.5e9
    assert [e["step"] for e in events[1:]] == [7, 8, 9] and all(e["file_version"] is None and e["wall_time"] > 1.5e9 for e in events[1:])
    assert SR.tags(events, 7) == ["generator_loss", "discriminator_loss"]
    assert SR.find(events, "generator_loss", 7)["simple_value"] == float(np.float32(0.1))
    assert SR.find(events, "discriminator_loss", 7)["simple_value"] == -2.5
    assert SR.tags(events, 8) == [f"{n}/image/{i}" for n in ("mag", "freq", "single") for i in range(3)]
    want = SR.images_u8(images.numpy())
    for c, n in enumerate(("mag", "freq")):
        for i in range(3):
            assert np.array_equal(SR.decode_png(SR.find(events, f"{n}/image/{i}", 8)), want[i, c]), (n, i)
    for i in range(3):
        assert np.array_equal(SR.decode_png(SR.find(events, f"single/image/{i}", 8)), want[i, 0])
    assert SR.tags(events, 9) == ["notes/audio/0", "notes/audio/1"]
    want = SR.audio_s16(audio.numpy())
    for i in range(2):
        rate, data = SR.decode_wav(SR.find(events, f"notes/audio/{i}", 9))
        assert rate == 16000 and np.array_equal(data, want[i])


def test_a_batch_of_six_gives_four_indexed_tags(tmp_path):
    from gansynth_amd import summary
    g = torch.Generator().manual_seed(5)
    with summary.SummaryWriter(str(tmp_path)) as w:
        w.images(1, {"x": torch.randn(6, 4, 8, generator=g)})
        w.audio(1, {"y": torch.rand(6, 50, generator=g) - 0.5}, 16000)
        path = w.path
    events = SR.read_events(path)
    assert SR.tags(events, 1) == [f"x/image/{i}" for i in range(4)] + [f"y/audio/{i}" for i in range(4)]


def test_no_record_no_file(tmp_path):
    from gansynth_amd import summary
    with summary.SummaryWriter(str(tmp_path)) as w:
        w.flush()
    assert _events_files(tmp_path) == []


def test_a_failure_on_the_writer_thread_reaches_the_caller(tmp_path, monkeypatch):
    import pytest
    from gansynth_amd import summary

    def broken(*args, **kwargs):
        raise OSError("no space left")

    with summary.SummaryWriter(str(tmp_path)) as w:
        w.scalars(1, dict(a=1.0))
        w.flush()
        monkeypatch.setattr(summary, "png_gray8", broken)   # the encoder runs on the writer thread
        w.images(2, {"x": torch.zeros(1, 2, 2)})
        with pytest.raises(RuntimeError, match="writer thread"):
            w.flush()
        monkeypatch.undo()
        w.scalars(3, dict(a=3.0))                            # the writer goes on
    assert [e["step"] for e in SR.read_events(w.path)] == [0, 1, 3]


# --------------------------------------------------------------------------------------------------------- host fallback
def test_host_rules_equal_the_restatement():
    from gansynth_amd import summary
    for name, x in SR.image_cases().items():
        for bf16 in (False, True):
            planes = (SR.to_bf16(x) if bf16 else x).transpose(0, 2, 1)[..., None]      # [N, C, P, 1]
            assert np.array_equal(summary.quantise_images_host(planes)[..., 0], SR.image_reference(name, bf16)), (name, bf16)
    audio = SR.audio_case()
    want = SR.audio_s16(audio)
    assert np.array_equal(summary.quantise_audio_host(audio), want)
    assert want[0, :10].tolist() == [32767, -32768, 32767, -32768, 0, 32767, -32768, 0, 0, 0]
    assert want[0, 10:14].tolist() == [1, 2, 3, 4] and want[0, 18:22].tolist() == [-1, -2, -3, -4]   # (k + 0.5) / 32768: away from zero
    assert np.array_equal(summary.quantise_audio_host(SR.to_bf16(audio)), SR.audio_s16(SR.to_bf16(audio)))


def test_image_rule_branches():
    """The restatement itself on values worked out by hand."""
    assert SR.image_u8(np.array([-1.0, 0.0, 0.5, 1.0], dtype=np.float32)).tolist() == [1, 128, 191, 255]      # 127 / 1, + 128
    assert SR.image_u8(np.array([0.0, 1.0, 2.0, 4.0], dtype=np.float32)).tolist() == [0, 63, 127, 255]         # 255 / 4
    assert SR.image_u8(np.array([-5e-7, 5e-7], dtype=np.float32)).tolist() == [128, 128]
    assert SR.image_u8(np.array([0.0, 5e-7], dtype=np.float32)).tolist() == [0, 0]
    assert SR.image_u8(np.array([np.nan, np.inf, -np.inf], dtype=np.float32)).tolist() == [255, 255, 255]
    assert SR.image_u8(np.array([np.nan, -2.0, np.inf, 1.0], dtype=np.float32)).tolist() == [255, 1, 255, 191]


# ---------------------------------------------------------------------------------------------------------- training run
def _model(seed=0, batches=3):
    """The reduced GAN of tests/test_reference_signatures_cpu.py::_model."""
    from gansynth_amd import variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict
    from oracle import torch_ref as R

    variables.set_default_store(variables.VariableStore(device="cpu", seed=seed))
    pg = PGGAN(min_resolution=[2, 16], max_resolution=[4, 32], min_channels=8, max_channels=16, growing_level=1.0)
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(4, 16, generator=g), torch.nn.functional.one_hot(torch.randint(0, 5, (4,), generator=g), 5).float(),
             torch.randn(4, 2, 4, 32, generator=g).clamp(-1, 1)) for _ in range(batches)]
    cur = [0, 0]

    def real_input_fn():
        if cur[0] >= 2 * batches:
            raise StopIteration
        cur[0] += 1
        return data[(cur[0] - 1) % batches][2], data[(cur[0] - 1) % batches][1]

    def fake_input_fn():
        cur[1] += 1
        return data[(cur[1] - 1) % batches][0]

    return GANSynth(pg.generator, pg.discriminator, real_input_fn, fake_input_fn, None, Dict(R.DEFAULT_HYPER)), data


def test_training_run_writes_summaries_and_keeps_its_trajectory(cpu_backend, tmp_path):
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    model, data = _model()
    model.train(model_dir=str(with_dir), config=None, total_steps=2, save_checkpoint_steps=1000, save_summary_steps=1, log_tensor_steps=100,
                log=None)
    plain, _ = _model()
    plain.train(model_dir=str(without_dir), config=None, total_steps=2, save_checkpoint_steps=1000, save_summary_steps=None,
                log_tensor_steps=100, log=None)
    assert _events_files(without_dir) == []
    assert torch.equal(model.g_params.flat, plain.g_params.flat) and torch.equal(model.d_params.flat, plain.d_params.flat)
    (path,) = _events_files(with_dir)
    SR.check_record_crcs(path)
    events = SR.read_events(path)
    assert events[0]["file_version"] == "brain.Event:2"
    names = ["real_magnitude_spectrograms", "real_instantaneous_frequencies", "fake_magnitude_spectrograms", "fake_instantaneous_frequencies"]
    for step in (1, 2):
        assert SR.tags(events, step) == [f"{n}/image/{i}" for n in names for i in range(4)] + ["generator_loss", "discriminator_loss"]
    assert not any("/audio/" in t for t in SR.tags(events))
    assert [e["step"] for e in events[1:]] == [1, 1, 2, 2]     # images, then scalars (no audio record: it would be empty)
    # the real side is the discriminator run's batch of that iteration: batch 0 at step 1, batch 2 at step 2 (_next_inputs)
    for step, batch in ((1, 0), (2, 2)):
        want = SR.images_u8(data[batch][2].numpy())
        assert np.array_equal(SR.decode_png(SR.find(events, "real_magnitude_spectrograms/image/3", step)), want[3, 0])
        assert np.array_equal(SR.decode_png(SR.find(events, "real_instantaneous_frequencies/image/0", step)), want[0, 1])
    # the fake side at the last step: the final generator over that iteration's generator-run latents and labels (the fourth call of
    # each input function: batch 3 % 3 = 0)
    with torch.no_grad():
        fake = model.generator(data[0][0], data[0][1])
    want = SR.images_u8(fake.float().numpy())
    assert np.array_equal(SR.decode_png(SR.find(events, "fake_magnitude_spectrograms/image/1", 2)), want[1, 0])
    assert SR.find(events, "generator_loss", 2)["simple_value"] == float(np.float32(float(model.generator_loss)))


# ------------------------------------------------------------------------------------------------------- the C ABI's checks
def test_entry_points_refuse_bad_arguments_without_a_launch():
    """Host-side checks of gs_summary_image_u8 / gs_summary_audio_s16 (no device needed: they return before any launch)."""
    from gansynth_amd import _lib
    lib = _lib.load()
    need = lib.gs_summary_image_u8_workspace_bytes(4, 128 * 1024, 2)
    assert need == 4 * 2 * 64 * 2 * 4                      # (min, max) per plane and 2048-pixel slab
    assert lib.gs_summary_image_u8_workspace_bytes(3, 5 * 37, 1) == 3 * 2 * 4
    assert lib.gs_summary_image_u8_workspace_bytes(4, 128, 3) == 0 and lib.gs_summary_image_u8_workspace_bytes(0, 128, 1) == 0
    x, out, ws = 0x10000, 0x20000, 0x30000                 # (never dereferenced)
    assert lib.gs_summary_image_u8(x, out, 4, 128 * 1024, 3, _lib.GS_F32, ws, need, None) == -1 and b"channels" in lib.gs_last_error()
    assert lib.gs_summary_image_u8(x, out, 4, 128 * 1024, 0, _lib.GS_BF16, ws, need, None) == -1
    assert lib.gs_summary_image_u8(x, out, 0, 128 * 1024, 2, _lib.GS_F32, ws, need, None) == -1
    assert lib.gs_summary_image_u8(x, out, -1, 128 * 1024, 2, _lib.GS_F32, ws, need, None) == -1
    assert lib.gs_summary_image_u8(x, out, 4, 128 * 1024, 2, _lib.GS_F32, ws, need - 1, None) == -1 and b"workspace" in lib.gs_last_error()
    assert lib.gs_summary_image_u8(x, out, 4, 128 * 1024, 2, _lib.GS_F32, None, 0, None) == -1
    assert lib.gs_summary_audio_s16(x, out, 0, 1003, 1003, _lib.GS_F32, None) == -1
    assert lib.gs_summary_audio_s16(x, out, 2, 1003, 1000, _lib.GS_F32, None) == -1 and b"stride" in lib.gs_last_error()
