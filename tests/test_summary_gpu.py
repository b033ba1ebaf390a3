"""GPU: gs_summary_image_u8 / gs_summary_audio_s16 against the restatement of tests/summary_ref.py -- exact equality: the arithmetic is
specified to the bit -- and the two trainers with summaries on: what the events file holds, and that the weights are those of a run
without summaries."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import torch_ref as R
from tests import summary_ref as SR

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]


def _K():
    from gansynth_amd import kernels
    return kernels.get()


def _image_u8(x, dtype):
    """The entry point itself on [N, P, C] (numpy float32) stored as `dtype`: uint8 [N, C, P]."""
    from gansynth_amd import _lib, kernels
    K = _K()
    n, p, c = x.shape
    dev = torch.from_numpy(x).cuda().to(dtype).contiguous()
    out = torch.full((n, c, p), 77, dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(K.lib.gs_summary_image_u8_workspace_bytes(n, p, c), 256), dtype=torch.uint8, device="cuda")
    _lib.check(K.lib.gs_summary_image_u8(dev.data_ptr(), out.data_ptr(), n, p, c, kernels._dt(dev), ws.data_ptr(), ws.numel(), kernels._stream()),
               "gs_summary_image_u8")
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(SR.image_cases()))
def test_image_kernel_equals_the_restatement(name, dtype):
    bf16 = dtype == torch.bfloat16
    got = _image_u8(SR.image_cases()[name], dtype)
    want = SR.image_reference(name, bf16)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_image_wrapper_layouts_and_count(dtype):
    """kernels.summary_image_u8: channels-last [B, 2, H, W] (both planes in one pass), [B, H, W], the first four items only."""
    g = torch.Generator().manual_seed(30)
    x = torch.randn(6, 2, 5, 37, generator=g)
    x[:, 1] = x[:, 1].abs()
    stored = x.to(dtype)
    want = SR.images_u8(stored.float().numpy())
    got = _K().summary_image_u8(stored.cuda().contiguous(memory_format=torch.channels_last))
    assert tuple(got.shape) == (4, 2, 5, 37) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want[:4])
    got = _K().summary_image_u8(stored.cuda())                       # (NCHW: the wrapper re-lays the four items it reads)
    assert np.array_equal(got.cpu().numpy(), want[:4])
    got = _K().summary_image_u8(stored[:, 0].cuda().contiguous(), count=2)
    assert tuple(got.shape) == (2, 1, 5, 37) and np.array_equal(got.cpu().numpy()[:, 0], want[:2, 0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_audio_kernel_equals_the_restatement(dtype):
    case = SR.audio_case()
    stored = torch.from_numpy(case).to(dtype)
    want = SR.audio_s16(stored.float().numpy())
    wide = torch.zeros(2, 1100, dtype=dtype)
    wide[:, :1003] = stored
    view = wide.cuda()[:, :1003]                                       # a row stride larger than L
    assert view.stride(0) == 1100
    got = _K().summary_audio_s16(view)
    assert tuple(got.shape) == (2, 1003) and got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(_K().summary_audio_s16(stored.cuda()).cpu().numpy(), want)
    # rows that are aligned for the packed path, more than one block per row, more rows than are wanted
    g = torch.Generator().manual_seed(31)
    long = ((torch.rand(5, 4096 + 8 * 13, generator=g) - 0.5) * 2.2).to(dtype)
    got = _K().summary_audio_s16(long.cuda())
    assert tuple(got.shape) == (4, long.shape[1]) and np.array_equal(got.cpu().numpy(), SR.audio_s16(long[:4].float().numpy()))


def test_device_and_host_paths_of_the_writer_agree(tmp_path):
    """SummaryWriter dispatches on tensor.is_cuda: the same tensors through the kernels and through the numpy statement, one file each."""
    from gansynth_amd import summary
    g = torch.Generator().manual_seed(32)
    images = torch.randn(5, 2, 16, 128, generator=g).contiguous(memory_format=torch.channels_last)
    audio = torch.from_numpy(SR.audio_case().copy())
    decoded = []
    for where, move in (("host", lambda t: t), ("device", lambda t: t.cuda())):
        with summary.SummaryWriter(str(tmp_path / where)) as w:
            w.audio(1, dict(a=move(audio)), 16000)
            w.images(1, {("m", "f"): move(images)})
            path = w.path
        SR.check_record_crcs(path)
        events = SR.read_events(path)
        assert SR.tags(events, 1) == ["a/audio/0", "a/audio/1"] + [f"{n}/image/{i}" for n in "mf" for i in range(4)]
        decoded.append([SR.decode_wav(v)[1] if "audio" in v else SR.decode_png(v) for e in events for v in e["values"]])
    assert all(np.array_equal(a, b) for a, b in zip(*decoded))
    assert np.array_equal(decoded[1][2], SR.images_u8(images.numpy())[0, 0])


# ---------------------------------------------------------------------------------------------------------- GANSynth.train
def _events_files(model_dir):
    return sorted(glob.glob(os.path.join(str(model_dir), "events.out.tfevents.*")))


def _gan(steps, spectral=None):
    """The reduced PGGAN of tests/test_model_gpu.py's train() tests, fully grown, batch 4, replaying graphs.  Without `spectral` the input
    gives images, with it waveforms.  Returns (model, the list of g-run (latents, labels) per iteration, the list of real batches)."""
    from gansynth_amd import variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    pg = PGGAN(growing_level=1.0, min_resolution=[2, 16], max_resolution=[16, 128], min_channels=32, max_channels=64)
    batches = [R.synthetic_batch(4, rank=i, image_shape=(2, 16, 128)) for i in range(2 * steps)]   # (latents, labels, real images)
    waves = torch.rand(2 * steps, 4, 1024, generator=torch.Generator().manual_seed(33)) - 0.5
    calls = {"real": 0, "fake": 0}
    g_inputs, reals = [], []

    def real_input_fn():   # D run: data + labels of batch 2i; G run: the labels of batch 2i + 1 (GANSynth._next_inputs)
        i = calls["real"]
        calls["real"] += 1
        data = waves[i].cuda() if spectral is not None else batches[i][2].cuda().contiguous(memory_format=torch.channels_last)
        if i % 2 == 0:
            reals.append(data)
        return data, batches[i][1].cuda()

    def fake_input_fn():
        i = calls["fake"]
        calls["fake"] += 1
        if i % 2 == 1:
            g_inputs.append((batches[i][0].cuda(), batches[i][1].cuda()))
        return batches[i][0].cuda()

    model = GANSynth(pg.generator, pg.discriminator, real_input_fn, fake_input_fn, spectral, Dict(R.DEFAULT_HYPER), use_graphs=True)
    return model, g_inputs, reals


def test_gan_training_with_summaries_keeps_the_weights_and_writes_the_images(tmp_path):
    steps = 3
    model, g_inputs, reals = _gan(steps)
    model.train(model_dir=str(tmp_path / "with"), config=None, total_steps=steps, save_checkpoint_steps=0, save_summary_steps=1,
                log_tensor_steps=100, log=None)
    plain, _, _ = _gan(steps)
    plain.train(model_dir=str(tmp_path / "without"), config=None, total_steps=steps, save_checkpoint_steps=0, save_summary_steps=None,
                log_tensor_steps=100, log=None)
    assert model._merged is not None or set(model._graphs) == {"d", "g"}           # (replaying captured iterations)
    assert torch.equal(model.g_params.flat, plain.g_params.flat) and torch.equal(model.d_params.flat, plain.d_params.flat)
    assert _events_files(tmp_path / "without") == []
    (path,) = _events_files(tmp_path / "with")
    events = SR.read_events(path)
    names = ["real_magnitude_spectrograms", "real_instantaneous_frequencies", "fake_magnitude_spectrograms", "fake_instantaneous_frequencies"]
    for step in range(1, steps + 1):
        assert SR.tags(events, step) == [f"{n}/image/{i}" for n in names for i in range(4)] + ["generator_loss", "discriminator_loss"]
    assert len(SR.tags(events)) == steps * (2 + 4 * 4)
    assert SR.find(events, "discriminator_loss", steps)["simple_value"] == float(np.float32(float(model.discriminator_loss)))
    with torch.no_grad():
        fake = model.generator(*g_inputs[steps - 1])
    want = SR.images_u8(fake.float().cpu().numpy())
    assert np.array_equal(SR.decode_png(SR.find(events, "fake_magnitude_spectrograms/image/0", steps)), want[0, 0])
    assert np.array_equal(SR.decode_png(SR.find(events, "fake_instantaneous_frequencies/image/3", steps)), want[3, 1])
    want = SR.images_u8(reals[steps - 1].float().cpu().numpy())
    assert np.array_equal(SR.decode_png(SR.find(events, "real_instantaneous_frequencies/image/2", steps)), want[2, 1])


def test_gan_audio_summaries(tmp_path):
    """The geometry of tests/test_model_gpu.py::test_generate_vs_oracle: 1024 samples <-> 16 x 128 images."""
    from gansynth_amd.utils import Dict
    spectral = Dict(waveform_length=1024, sample_rate=16000, spectrogram_shape=[16, 128], overlap=0.75)
    model, g_inputs, reals = _gan(1, spectral)
    model.train(model_dir=str(tmp_path), config=None, total_steps=1, save_checkpoint_steps=0, save_summary_steps=1, log_tensor_steps=100, log=None)
    (path,) = _events_files(tmp_path)
    events = SR.read_events(path)
    assert [e["step"] for e in events] == [0, 1, 1, 1]                             # version, then audio, images, scalars
    assert SR.tags(events, 1)[:8] == [f"{n}/audio/{i}" for n in ("real_waveforms", "fake_waveforms") for i in range(4)]
    want = SR.audio_s16(model.generate(*g_inputs[0])[0].float().cpu().numpy())
    rate, got = SR.decode_wav(SR.find(events, "fake_waveforms/audio/0", 1))
    assert rate == 16000 and np.array_equal(got, want)
    rate, got = SR.decode_wav(SR.find(events, "real_waveforms/audio/3", 1))
    assert rate == 16000 and np.array_equal(got, SR.audio_s16(reals[0][3].cpu().numpy()))


# ------------------------------------------------------------------------------------------------------ PitchClassifier.train
def _classifier(seed=90):
    """The reduced ResNet of tests/test_classifier_train_gpu.py (two stages, 64 and 128 filters) on 2048-sample notes <-> 32 x 128 images."""
    from gansynth_amd import variables
    from gansynth_amd.models import PitchClassifier
    from gansynth_amd.networks import ResNet
    from gansynth_amd.utils import Dict
    net = ResNet(conv_param=Dict(filters=64, kernel_size=[7, 7], strides=[2, 2]), pool_param=Dict(kernel_size=[3, 3], strides=[2, 2]),
                 residual_params=[Dict(filters=f, strides=[s, s], blocks=b) for f, s, b in [(64, 1, 2), (128, 2, 1)]], groups=32, classes=61,
                 store=variables.VariableStore(device="cuda", seed=0))
    g = torch.Generator().manual_seed(seed)
    fed = []

    def input_fn():
        wav = (torch.rand(2, 2048, generator=g) - 0.5).cuda()
        fed.append(wav)
        return wav, torch.eye(61)[torch.randint(0, 61, (2,), generator=g)].cuda()

    hyper = Dict(weight_decay=1e-2, learning_rate=lambda step: 0.05 * 0.5 ** step, momentum=0.9, use_nesterov=True)
    spectral = Dict(waveform_length=2048, sample_rate=16000, spectrogram_shape=[32, 128], overlap=0.75)
    return PitchClassifier(net, input_fn, spectral, hyper), fed


def test_classifier_training_with_summaries(tmp_path):
    from gansynth_amd import spectral_ops
    lines = []
    model, fed = _classifier()
    model.train(str(tmp_path / "with"), None, 2, 100, 1, 1, log=lines.append)
    plain, _ = _classifier()
    plain.train(str(tmp_path / "without"), None, 2, 100, 0, 100, log=None)
    a, b = model.state_dict(), plain.state_dict()
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert _events_files(tmp_path / "without") == []
    (path,) = _events_files(tmp_path / "with")
    SR.check_record_crcs(path)
    events = SR.read_events(path)
    for step in (1, 2):
        assert SR.tags(events, step) == ([f"waveforms/audio/{i}" for i in range(2)]
                                         + [f"{n}/image/{i}" for n in ("magnitude_spectrograms", "instantaneous_frequencies") for i in range(2)]
                                         + ["loss", "accuracy"])
    # the values are the step's own batch and the log line's numbers
    _, got = SR.decode_wav(SR.find(events, "waveforms/audio/1", 2))
    assert np.array_equal(got, SR.audio_s16(fed[1][1].cpu().numpy()))
    images = spectral_ops.convert_to_images(fed[1], **model.spectral_params)
    assert np.array_equal(SR.decode_png(SR.find(events, "instantaneous_frequencies/image/0", 2)), SR.images_u8(images.cpu().numpy())[0, 1])
    for name in ("loss", "accuracy"):   # the log line prints six decimals of the float64 value, the event holds its float32
        logged = float(lines[1].split(f"{name} = ")[1].split(",")[0])
        assert abs(SR.find(events, name, 2)["simple_value"] - logged) <= 1e-6 * max(1.0, abs(logged)), name
