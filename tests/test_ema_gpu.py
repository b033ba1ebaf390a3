"""GPU: the averaged generator on the device -- gs_ema_step, gs_ema_step_dev and gs_swap_f32 element by element against float64
(tests/ema_ref.py), the trainer's average through the eager and the captured iteration forms, the three consumers, checkpoints, and the
driver's flags end to end.

Kernel bound: |got - ref| <= 3 * 2^-24 * max(|s|, |w|, |ref|) per element.  The kernel rounds twice -- the difference d = s - w (error
<= 2^-24 |d| <= 2^-24 * 2 max(|s|, |w|)) and one fused multiply-add (error <= 2^-24 |result|) -- and one_minus <= 1 scales the first.
The bound is relative, so it says nothing below the normal range: a denormal is paired with a normal partner on either side (the bound is
then the partner's), or with itself (the result is exact); two DIFFERENT denormals would be held to less than their own spacing.  |s - w|
beyond FLT_MAX overflows in fp32 as it does in TF: the +-3e38 rows keep their differences finite."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import torch_ref as R
from tests import ema_ref as ER

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVG = "/ExponentialMovingAverage"
EPS = 2.0 ** -24
GUARD = 8
# 8192 * 256 * 4 + 5: the smallest size at which the grid-stride loop takes a second sweep under ew_grid's cap of 8192 blocks, plus a tail
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 64 * 1000, 8192 * 256 * 4 + 5]
ONE_MINUS = [0.0, 2.0 ** -10, 0.001, 0.5, 1.0]
NAN_AT, INF_AT = 100, 101


@pytest.fixture(scope="module")
def K():
    from gansynth_amd import kernels
    return kernels.get()


def inputs(n, seed=0):
    """(shadow, p) fp32 numpy: normal values; from 255 elements on also a block of exact zeros, denormals, +-3e38, one NaN and one inf in p."""
    rng = np.random.default_rng(seed + n)
    s, w = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    if n >= 255:
        s[10:40] = 0.0
        w[10:30] = 0.0                                          # zeros on both sides; zeros against values, both ways
        w[40:50] = 0.0
        den = (np.arange(1, 11) * 1.0e-40).astype(np.float32)   # denormals (below 1.18e-38)
        assert np.all(den > 0) and np.all(den < np.finfo(np.float32).tiny)
        s[60:70] = den                                          # against a normal partner, both ways, and against themselves
        w[70:80] = -den
        s[80:90] = w[80:90] = den
        s[90:95] = [3e38, -3e38, 3e38, 1.0, -3e38]
        w[90:95] = [3e38, -3e38, 1.0, -3e38, -2.5]
        w[NAN_AT], w[INF_AT] = np.nan, np.inf
    return s, w


def guarded(values):
    """A device buffer with GUARD floats of a known pattern on either side of `values`; returns (whole buffer, the 16-byte aligned view)."""
    buf = torch.full((GUARD + len(values) + GUARD,), -12345.5, dtype=torch.float32, device="cuda")
    view = buf[GUARD:GUARD + len(values)]
    view.copy_(torch.from_numpy(values))
    assert view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf):
    return bool((buf[:GUARD] == -12345.5).all()) and bool((buf[-GUARD:] == -12345.5).all())


def check_step(got, s, w, om, what, steps=1):
    ref = ER.step(s, w, om)
    got = got.astype(np.float64)
    special = ~np.isfinite(w.astype(np.float64))
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), what
    if om > 0:
        assert np.array_equal(~np.isfinite(got), special), f"{what}: the NaN and the inf of p reach the shadow at their own indices only"
    ok = np.isfinite(ref)
    scale = np.maximum(np.maximum(np.abs(s.astype(np.float64)), np.abs(w.astype(np.float64))), np.abs(ref))
    err = np.abs(got[ok] - ref[ok])
    excess = err - steps * 3.0 * EPS * scale[ok]
    worst = float(np.max(err / np.maximum(scale[ok], 1e-300))) / EPS if ok.any() else 0.0
    assert np.all(excess <= 0), f"{what}: worst error {worst:.3f} x 2^-24 of the element's scale (bound {3 * steps})"
    return worst


@pytest.mark.parametrize("n", SIZES)
def test_ema_step_against_float64(K, n):
    s, w = inputs(n)
    worst = 0.0
    for om in ONE_MINUS:
        sbuf, sv = guarded(s)
        wbuf, wv = guarded(w)
        K.ema_step(sv, wv, om)
        got = sv.cpu().numpy()
        assert guards_intact(sbuf) and guards_intact(wbuf), (n, om)
        assert np.array_equal(wv.cpu().numpy().view(np.int32), w.view(np.int32))          # p is read only
        if om == 0.0:
            assert np.array_equal(got.view(np.int32), s.view(np.int32)), n               # a decay of 1: every bit stays
            continue
        worst = max(worst, check_step(got, s, w, om, f"n = {n}, one_minus = {om}"))
        if om == 1.0:   # the shadow becomes p (within the same bound: the difference is rounded)
            ok = np.isfinite(w)
            scale = np.maximum(np.abs(s[ok].astype(np.float64)), np.abs(w[ok].astype(np.float64)))
            assert np.all(np.abs(got[ok].astype(np.float64) - w[ok]) <= 3.0 * EPS * scale)
    print(f"gs_ema_step n = {n}: worst error {worst:.3f} x 2^-24 of the element's scale")


@pytest.mark.parametrize("n", [3, 257, 64 * 1000])
def test_ema_step_dev_reads_its_scalar_when_it_runs(K, n):
    from gansynth_amd import functional as F
    s, w = inputs(n)
    table = F.DeviceScalars("cuda", 2)
    for om in ONE_MINUS[1:]:
        table.set([om, -1.0])
        sbuf, sv = guarded(s)
        wbuf, wv = guarded(w)
        K.ema_step_dev(sv, wv, table.ptr(0))
        got = sv.cpu().numpy()
        assert guards_intact(sbuf) and guards_intact(wbuf)
        check_step(got, s, w, om, f"dev, n = {n}, one_minus = {om}")
        _, by_value = guarded(s)
        K.ema_step(by_value, wv, om)
        assert np.array_equal(by_value.cpu().numpy().view(np.int32), got.view(np.int32))   # the same arithmetic on the same fp32 scalar
    # a negative scalar: no step pending -- a NaN-prefilled shadow keeps every bit
    pattern = np.full(n, 0x7FC12345, dtype=np.int32)
    pattern[::2] = -4194303                                       # 0xFFC00001: another payload, sign set
    sbuf, sv = guarded(pattern.view(np.float32))
    _, wv = guarded(w)
    K.ema_step_dev(sv, wv, table.ptr(1))
    assert np.array_equal(sv.cpu().numpy().view(np.int32), pattern) and guards_intact(sbuf)
    # inside a captured graph the scalar is read at replay time: 0.5, then nothing, then 0.25 -- the two-step recurrence
    s, w = inputs(n, seed=1)
    finite = np.where(np.isfinite(w), w, np.float32(0.5))          # (two steps: keep the reference's special values out of the second)
    sbuf, sv = guarded(s)
    _, wv = guarded(finite)
    table.set([-1.0, -1.0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.ema_step_dev(sv, wv, table.ptr(0))
    for om in (0.5, -1.0, 0.25):
        table.set([om, -1.0])
        graph.replay()
    torch.cuda.synchronize()
    twice = ER.step(ER.step(s, finite, 0.5), finite, 0.25)          # (float64 throughout; the middle replay changed nothing)
    got = sv.cpu().numpy().astype(np.float64)
    # two steps: the first one's error (<= 3 * 2^-24 of the scale) is carried with a factor 1 - 0.25, the second adds its own
    scale = np.maximum(np.maximum(np.abs(s.astype(np.float64)), np.abs(finite.astype(np.float64))), np.abs(twice))
    assert np.all(np.abs(got - twice) <= 2 * 3.0 * EPS * scale)
    assert guards_intact(sbuf)


@pytest.mark.parametrize("n", SIZES)
def test_swap_moves_bits(K, n):
    rng = np.random.default_rng(n)
    a = rng.integers(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int64).astype(np.int32)   # any bit pattern: NaN payloads, denormals, infinities
    b = rng.integers(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int64).astype(np.int32)
    a[0] = np.int32(-2 ** 31)                                                      # -0.0
    if n > 4:
        a[1], a[2], b[3], b[4] = 0x7FC12345, 0x7F800001, -4194303, 0               # quiet and signalling NaNs with payloads, +0.0
    abuf, av = guarded(a.view(np.float32))
    bbuf, bv = guarded(b.view(np.float32))
    K.swap_(av, bv)
    assert np.array_equal(av.cpu().numpy().view(np.int32), b) and np.array_equal(bv.cpu().numpy().view(np.int32), a)
    assert guards_intact(abuf) and guards_intact(bbuf)
    K.swap_(av, bv)
    assert np.array_equal(av.cpu().numpy().view(np.int32), a) and np.array_equal(bv.cpu().numpy().view(np.int32), b)
    assert guards_intact(abuf) and guards_intact(bbuf)


# ------------------------------------------------------------------------------------------------------------ the trainer
LR = 5e-3   # (see tests/test_ema_cpu.py: the weights must move by at least 100 bounds, asserted)
SPECTRAL = dict(waveform_length=1024, sample_rate=16000, spectrogram_shape=[16, 128], overlap=0.75)


def use(model):
    from gansynth_amd import variables
    variables.set_default_store(model.store)
    return model


def make_model(decay=None, dtype=torch.float32, graphs=False, level=1.0, seed=0, batches=8):
    """The reduced PGGAN of tests/test_model_gpu.py (2x16 -> 16x128, 32..64 channels) at batch 4, inputs that never run dry."""
    from gansynth_amd import variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict
    variables.set_default_store(variables.VariableStore(device="cuda", seed=seed))
    pg = PGGAN(growing_level=level, min_resolution=[2, 16], max_resolution=[16, 128], min_channels=32, max_channels=64)
    data = [R.synthetic_batch(4, rank=i, image_shape=(2, 16, 128)) for i in range(batches)]   # (latents, labels, real images)
    cur = [0, 0]

    def real_input_fn():
        cur[0] += 1
        _, labels, real = data[(cur[0] - 1) % batches]
        return real.cuda().contiguous(memory_format=torch.channels_last), labels.cuda()

    def fake_input_fn():
        cur[1] += 1
        return data[(cur[1] - 1) % batches][0].cuda()

    hyper = dict(R.DEFAULT_HYPER, generator_learning_rate=LR, discriminator_learning_rate=LR)
    if decay is not None:
        hyper["generator_average_decay"] = decay
    model = GANSynth(pg.generator, pg.discriminator, real_input_fn, fake_input_fn, Dict(SPECTRAL), Dict(hyper), dtype=dtype, use_graphs=graphs)
    return model, data


def build(model, data):
    use(model)._build(data[0][0].cuda().to(model.dtype), data[0][1].cuda().to(model.dtype))
    return model


def ranges(params):
    return [((p.data.data_ptr() - params.flat.data_ptr()) // 4, p.numel()) for p in params.named.values()]


def train(model, steps, snapshots=None, before_step=None):
    """`steps` train_steps WITHOUT joining in between (the one-graph iteration keeps the generator's step pending: the next replay applies
    it), then synchronize().  `snapshots` receives the generator's weights after each of its steps, taken when that step has been applied."""
    use(model)
    losses = []

    def snap():
        applied = model.g_params.t - (1 if model._g_pending is not None else 0)
        if snapshots is not None and applied == len(snapshots):
            snapshots.append(model.g_params.flat.detach().clone())

    for i in range(steps):
        if before_step is not None:
            before_step(i)
        d, g = model.train_step()
        losses.append((d.detach().clone(), g.detach().clone()))
        snap()
    model.synchronize()
    snap()
    return losses


def same_trajectory(a, b, losses_a, losses_b):
    for i, ((d0, g0), (d1, g1)) in enumerate(zip(losses_a, losses_b)):
        assert torch.equal(d0, d1) and torch.equal(g0, g1), f"losses of step {i}"
    for pa, pb in ((a.g_params, b.g_params), (a.d_params, b.d_params)):
        assert torch.equal(pa.flat, pb.flat) and torch.equal(pa.m, pb.m) and torch.equal(pa.v, pb.v) and pa.t == pb.t
    assert a.global_step == b.global_step


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_trainer_average_is_an_observer_and_follows_the_recurrence(K, dtype, graphs):
    """Six steps: eagerly, six by-value updates; with graphs on one GPU the one-graph iteration -- the capture, the first replay's skipped
    step, five replays that apply a pending step with its update of the average behind it, and the final join by value."""
    plain, data = make_model(None, dtype, graphs)
    plain_losses = train(plain, 6)
    by_value, in_graph = K.ema_steps, K.ema_steps_dev
    model, _ = make_model(0.999, dtype, graphs)
    build(model, data)
    snapshots = [model.g_params.flat.detach().clone()]
    assert torch.equal(model.g_params.avg, snapshots[0])
    losses = train(model, 6, snapshots)
    assert len(snapshots) == 7
    # the HIP path, not the torch expression: the wrappers counted
    assert hasattr(K, "ema_step") and hasattr(K, "ema_step_dev")
    if graphs:
        assert model._merged is not None and model._merged["fused"], "one GPU with graphs: the one-graph iteration"
        assert K.ema_steps_dev - in_graph == 1 and K.ema_steps - by_value == 1   # one captured node; the final join by value
    else:
        assert K.ema_steps_dev == in_graph and K.ema_steps - by_value == 6
    same_trajectory(plain, model, plain_losses, losses)
    assert plain.g_params.avg is None and model.d_params.avg is None
    ER.check_recurrence(snapshots, model.g_params.avg, 0.999, ranges(model.g_params), f"{dtype}, graphs = {graphs}")


def test_trainer_average_across_a_recapture_in_a_fade_in_regime(K):
    """The growing regime of tests/test_model_gpu.py::test_hipgraph_replay_in_a_fade_in_regime, three steps: depth 2.0 (fading), then 2.15
    and 2.29 (the next head: a re-capture, which joins the pending step by value, then a replay that applies one in the graph)."""
    out = {}
    for decay in (None, 0.999):
        step = [0]
        model, data = make_model(decay, torch.float32, True, level=lambda: 0.20 + 0.03 * step[0])
        build(model, data)
        snapshots = [model.g_params.flat.detach().clone()]
        keys = []

        def before(i):
            step[0] = i
            keys.append(model._regime()[0])
        losses = train(model, 3, snapshots, before_step=before)
        assert len(set(keys)) == 2 and keys[0] != keys[1], keys           # a re-capture in between
        out[decay] = (model, losses, snapshots)
    same_trajectory(out[None][0], out[0.999][0], out[None][1], out[0.999][1])
    model, _, snapshots = out[0.999]
    assert len(snapshots) == 4
    ER.check_recurrence(snapshots, model.g_params.avg, 0.999, ranges(model.g_params), "fade-in regime, re-capture")


# ------------------------------------------------------------------------------------------------------------ consumers
def _second_model_from_the_shadow(model, data):
    from gansynth_amd import checkpoint
    state = checkpoint.state_dict(model)
    for name in model.g_params.named:
        state[name] = state.pop(name + AVG)
    second, _ = make_model(None, model.dtype, seed=7)
    build(second, data)
    checkpoint.load_state_dict(second, state)
    return second


def _score():
    from gansynth_amd.notes import Note
    return [Note(60, 100, 0.0, 0.02), Note(64, 80, 0.01, 0.05), Note(31, 127, 0.03, 0.04)]


def _evaluate_inputs(model, data):
    """A finite two-batch input of images for evaluate, and a small ResNet (two stages) in a store of its own."""
    from gansynth_amd import variables
    from gansynth_amd.networks import ResNet
    from gansynth_amd.utils import Dict
    cur = [0, 0]

    def real_input_fn():
        if cur[0] >= 2:
            raise StopIteration
        cur[0] += 1
        _, labels, real = data[cur[0] - 1]
        return real.cuda().contiguous(memory_format=torch.channels_last), labels.cuda()

    def fake_input_fn():
        cur[1] += 1
        return data[cur[1] - 1][0].cuda()

    model.real_input_fn, model.fake_input_fn = real_input_fn, fake_input_fn
    return ResNet(conv_param=Dict(filters=64, kernel_size=[7, 7], strides=[2, 2]), pool_param=Dict(kernel_size=[3, 3], strides=[2, 2]),
                  residual_params=[Dict(filters=f, strides=[s, s], blocks=b) for f, s, b in [(64, 1, 2), (128, 2, 1)]], groups=32, classes=61,
                  store=variables.VariableStore(device="cuda", seed=0))


def test_consumers_read_the_average_and_leave_the_model_alone():
    model, data = make_model(0.999, graphs=True)
    train(model, 3)
    second = _second_model_from_the_shadow(model, data)
    assert torch.equal(second.g_params.flat, model.g_params.avg) and not torch.equal(model.g_params.flat, model.g_params.avg)
    lat, lab = data[1][0].cuda(), data[1][1].cuda()
    kw = dict(normalize=False, batch_size=4, release_seconds=0.01, seconds_per_instrument=0.04, seed=2)
    want_wave, want_clip = use(second).generate(lat, lab), second.synthesize(_score(), **kw)
    second_features = {}
    want_fid = second.evaluate(None, None, _evaluate_inputs(second, data), features_out=second_features, batch_size=4)
    use(model)
    flat, avg = model.g_params.flat.clone(), model.g_params.avg.clone()
    cpu_rng, gpu_rng = torch.random.get_rng_state(), torch.cuda.get_rng_state()
    wave = model.generate(lat, lab, weights="average")
    assert torch.equal(wave, want_wave) and not torch.equal(wave, model.generate(lat, lab))
    clip = model.synthesize(_score(), weights="average", **kw)
    assert torch.equal(clip, want_clip) and not torch.equal(clip, model.synthesize(_score(), **kw))
    kept = model.real_input_fn, model.fake_input_fn
    features = {}
    fid = model.evaluate(None, None, _evaluate_inputs(model, data), features_out=features, batch_size=4, weights="average")
    model.real_input_fn, model.fake_input_fn = kept
    assert sorted(features) == sorted(second_features) and all(np.array_equal(features[k], second_features[k]) for k in features)
    a, b = fid["frechet_inception_distance"], want_fid["frechet_inception_distance"]
    assert a == b or (np.isnan(a) and np.isnan(b))
    assert torch.equal(model.g_params.flat, flat) and torch.equal(model.g_params.avg, avg) and not model._average_in
    assert torch.equal(torch.random.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
    # a following train_step equals the one of a model that never looked at its average (its captured graph still holds valid pointers)
    never, _ = make_model(0.999, graphs=True)
    train(never, 3)
    a = train(model, 1)
    b = train(never, 1)
    same_trajectory(model, never, a, b)
    assert torch.equal(model.g_params.avg, never.g_params.avg)


def test_no_average_to_read_is_an_error_and_the_context_refuses_training(tmp_path):
    from gansynth_amd import checkpoint
    off, data = make_model(None)
    train(off, 1)
    first = next(iter(off.g_params.named)) + AVG
    lat, lab = data[0][0].cuda(), data[0][1].cuda()
    with pytest.raises(ValueError, match=first):
        off.generate(lat, lab, weights="average")
    checkpoint.save(off, str(tmp_path / "off"))
    with pytest.raises(ValueError, match=first):
        off.synthesize(_score(), model_dir=str(tmp_path / "off"), weights="average", batch_size=4, release_seconds=0.01)
    assert off.g_params.avg is None
    on, _ = make_model(0.999)
    train(on, 2)
    flat, avg = on.g_params.flat.clone(), on.g_params.avg.clone()
    with on.averaged_generator():
        assert torch.equal(on.g_params.flat, avg) and torch.equal(on.g_params.avg, flat)
        for call in (on.train_step, lambda: checkpoint.save(on, str(tmp_path / "never")), lambda: checkpoint.state_dict(on)):
            with pytest.raises(RuntimeError, match="average is swapped in"):
                call()
    with pytest.raises(KeyError):
        with on.averaged_generator():
            raise KeyError("from the body")
    assert torch.equal(on.g_params.flat, flat) and torch.equal(on.g_params.avg, avg) and not on._average_in


def test_checkpoint_round_trip_on_the_device(tmp_path):
    from gansynth_amd import checkpoint
    model, _ = make_model(0.999, graphs=True)
    train(model, 2)
    flat, avg = model.g_params.flat.clone(), model.g_params.avg.clone()
    path = checkpoint.save(model, str(tmp_path))
    from safetensors.torch import load_file
    keys = set(load_file(path))
    assert {name + AVG for name in model.g_params.named} <= keys and not any(k.startswith("discriminator") and k.endswith(AVG) for k in keys)
    for name, p in model.g_params.named.items():   # (the variables, not the padding between them: that is zero in both buffers and stays zero)
        p.data.add_(0.25)
        model.g_params.avg_view(name).mul_(-3.0)
    assert not torch.equal(model.g_params.flat, flat) and not torch.equal(model.g_params.avg, avg)
    checkpoint.restore(model, str(tmp_path))
    assert torch.equal(model.g_params.flat, flat) and torch.equal(model.g_params.avg, avg)
    train(model, 1)   # (the restored model trains on: its graph's pointers and prepared operands are current)


# --------------------------------------------------------------------------------------------------------------- the driver
def test_driver_trains_with_an_average_and_generates_from_it(tmp_path):
    """`gan_synth_main.py --train --synthetic --total_steps 20 --generator_ema_decay 0.999`, then `--generate --weights average
    --num_generate_batches 1` on that directory, each in a fresh process (the full-size model: what the driver builds)."""
    from safetensors.torch import load_file
    from scipy.io import wavfile
    main = os.path.join(ROOT, "gan_synth_main.py")
    common = [sys.executable, main, "--synthetic", "--model_dir", str(tmp_path / "model"), "--save_summary_steps", "0"]
    r = subprocess.run(common + ["--train", "--total_steps", "20", "--generator_ema_decay", "0.999"], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "stopped at global_step = 20" in r.stdout
    state = load_file(str(tmp_path / "model" / "model.ckpt-20.safetensors"))
    averaged = [k for k in state if k.endswith(AVG)]
    assert averaged and all(k.startswith("generator/") and tuple(state[k].shape) == tuple(state[k[:-len(AVG)]].shape) for k in averaged)
    assert any(not torch.equal(state[k], state[k[:-len(AVG)]]) for k in averaged)
    r = subprocess.run(common + ["--generate", "--weights", "average", "--num_generate_batches", "1"], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "restored " in r.stdout and "8 waveforms are generated" in r.stdout
    rate, wave = wavfile.read(str(tmp_path / "samples" / "0.wav"))
    assert rate == 16000 and wave.shape == (64000,) and np.all(np.isfinite(wave))
