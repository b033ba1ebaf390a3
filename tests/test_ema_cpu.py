"""CPU: the averaged generator (hyper_params.generator_average_decay) on the emulation backend -- the reduced 2x16 model at batch 4 --
plus the host-side refusals of gs_ema_step / gs_ema_step_dev / gs_swap_f32 and the driver's flags.  The float64 restatement is
tests/ema_ref.py; the backend has no ema_step, so the trainer takes the torch expression of the same rule here."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ema_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVG = "/ExponentialMovingAverage"
LR = 5e-3          # (both networks) six Adam steps of ~lr each move the median weight by ~1e-2: thousands of bounds (asserted)
STEPS = 6


def make_model(decay=None, seed=0, lr=LR, device="cpu", batches=4):
    """The reduced GAN (2x16 -> 4x32, 8..16 channels, 256 latents, 61 pitches) at batch 4 on images, inputs that never run dry."""
    from gansynth_amd import variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict
    from oracle import torch_ref as R
    variables.set_default_store(variables.VariableStore(device=device, seed=seed))
    pg = PGGAN(min_resolution=[2, 16], max_resolution=[4, 32], min_channels=8, max_channels=16, growing_level=1.0)
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(4, 256, generator=g), torch.nn.functional.one_hot(torch.randint(0, 61, (4,), generator=g), 61).float(),
             torch.randn(4, 2, 4, 32, generator=g).clamp(-1, 1)) for _ in range(batches)]
    cur = [0, 0]

    def real_input_fn():
        cur[0] += 1
        return data[(cur[0] - 1) % batches][2].to(device), data[(cur[0] - 1) % batches][1].to(device)

    def fake_input_fn():
        cur[1] += 1
        return data[(cur[1] - 1) % batches][0].to(device)

    hyper = dict(R.DEFAULT_HYPER, generator_learning_rate=lr, discriminator_learning_rate=lr)
    if decay is not None:
        hyper["generator_average_decay"] = decay
    model = GANSynth(pg.generator, pg.discriminator, real_input_fn, fake_input_fn, None, Dict(hyper))
    return model, data


def use(model):
    """The networks look their variables up in the DEFAULT store: with several models alive, the one about to run owns it."""
    from gansynth_amd import variables
    variables.set_default_store(model.store)
    return model


def build(model, data):
    use(model)._build(data[0][0], data[0][1])
    return model


def ranges(params):
    return [((p.data.data_ptr() - params.flat.data_ptr()) // 4, p.numel()) for p in params.named.values()]


def train(model, steps=STEPS, snapshots=None):
    losses = []
    use(model)
    for _ in range(steps):
        d, g = model.train_step()
        model.synchronize()
        losses.append((torch.as_tensor(d).detach().clone(), torch.as_tensor(g).detach().clone()))
        if snapshots is not None:
            snapshots.append(model.g_params.flat.detach().clone())
    return losses


# ------------------------------------------------------------------------------------------------- 1, 2: observer, recurrence
def test_averaging_is_an_observer_and_follows_the_recurrence(cpu_backend):
    plain, _ = make_model(None)
    plain_losses = train(plain)
    model, data = make_model(0.999)
    build(model, data)
    assert plain.g_params.avg is None and plain.average_decay == 0.0
    assert torch.equal(model.g_params.avg, model.g_params.flat) and model.d_params.avg is None   # from the initial weights; the generator's only
    snapshots = [model.g_params.flat.detach().clone()]
    losses = train(model, snapshots=snapshots)
    for i, ((d0, g0), (d1, g1)) in enumerate(zip(plain_losses, losses)):
        assert torch.equal(d0, d1) and torch.equal(g0, g1), i
    for a, b in ((plain.g_params, model.g_params), (plain.d_params, model.d_params)):
        assert torch.equal(a.flat, b.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and a.t == b.t == STEPS
    assert plain.global_step == model.global_step == STEPS
    ER.check_recurrence(snapshots, model.g_params.avg, 0.999, ranges(model.g_params), "cpu emulation")


# ------------------------------------------------------------------------------------------------------------- 3: warm-up
def test_warm_up_against_the_closed_form(cpu_backend):
    from fractions import Fraction
    model, _ = make_model(0.999)
    for t in (1, 2, 90, 8990, 8991, 10 ** 6):
        warm = Fraction(9, 10 + t)                 # 1 - (1 + t) / (10 + t), exactly
        constant = 1 - Fraction(0.999)             # 1 - the double the decay is
        want = float(np.float32(float(max(warm, constant))))   # min of the decays = max of their complements
        assert ER.one_minus(0.999, t) == want, t
        assert model._one_minus(t) == want, t
        assert np.float32(model._one_minus(t)) == model._one_minus(t)   # an fp32 value
    # the cross-over: (1 + t) / (10 + t) passes 0.999 between t = 8990 (8991 / 9000, still the warm-up's value) and 8991 (the constant)
    assert 8991.0 / 9000.0 <= 0.999 < 8992.0 / 9001.0   # (as doubles, the arithmetic the trainer does)
    assert ER.one_minus(0.999, 8990) == float(np.float32(float(Fraction(9, 9000))))
    assert ER.one_minus(0.999, 8991) == float(np.float32(1.0 - 0.999)) != float(np.float32(float(Fraction(9, 9001))))
    assert ER.one_minus(0.999, 1) == float(np.float32(9.0 / 11.0)) and ER.one_minus(0.999, 2) == 0.75


# --------------------------------------------------------------------------------------------------------- 4: checkpoints
def _same_model(a, b):
    return all(torch.equal(x, y) for pa, pb in ((a.g_params, b.g_params), (a.d_params, b.d_params))
               for x, y in ((pa.flat, pb.flat), (pa.m, pb.m), (pa.v, pb.v))) and a.global_step == b.global_step


def test_checkpoint_keys_and_round_trips(cpu_backend, tmp_path):
    from gansynth_amd import checkpoint
    off, data = make_model(None)
    train(off, 2)
    model, _ = make_model(0.999)
    train(model, 2)
    today = set(checkpoint.state_dict(off))
    assert not any(k.endswith(AVG) for k in today)
    with_avg = checkpoint.state_dict(model)
    assert set(with_avg) == today | {name + AVG for name in model.g_params.named}
    for name, p in model.g_params.named.items():
        assert tuple(with_avg[name + AVG].shape) == tuple(p.shape) and torch.equal(with_avg[name + AVG], model.g_params.avg_view(name))
    # (a variable no regime reached has no gradient: its average IS its value; most differ)
    assert sum(not torch.equal(with_avg[name + AVG], with_avg[name]) for name in model.g_params.named) > len(model.g_params.named) // 2
    # a round trip restores the shadow bit for bit
    checkpoint.save(model, str(tmp_path / "on"))
    again, _ = make_model(0.999, seed=9)
    build(again, data)
    assert not torch.equal(again.g_params.avg, model.g_params.avg)
    checkpoint.restore(again, str(tmp_path / "on"))
    assert torch.equal(again.g_params.avg, model.g_params.avg) and _same_model(again, model)
    # saved with averaging OFF, restored into a model with it ON: the shadow starts at the restored weights, nothing is missing
    checkpoint.save(off, str(tmp_path / "off"))
    fresh, _ = make_model(0.999, seed=9)
    build(fresh, data)
    assert checkpoint.load_state_dict(fresh, checkpoint.state_dict(off), strict=True) == []
    assert torch.equal(fresh.g_params.avg, off.g_params.flat) and torch.equal(fresh.g_params.flat, off.g_params.flat)
    # a wrong-shaped average is refused and the model is as it was, bit for bit
    bad = dict(with_avg)
    name = next(iter(model.g_params.named))
    bad[name + AVG] = torch.zeros(tuple(with_avg[name].shape) + (2,))
    before = [t.clone() for t in (fresh.g_params.flat, fresh.g_params.avg, fresh.g_params.m, fresh.d_params.flat, fresh.d_params.v)]
    step = fresh.global_step
    with pytest.raises(ValueError, match="ExponentialMovingAverage"):
        checkpoint.load_state_dict(fresh, bad)
    after = (fresh.g_params.flat, fresh.g_params.avg, fresh.g_params.m, fresh.d_params.flat, fresh.d_params.v)
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and fresh.global_step == step
    # a model without a shadow restores a file that has averages and ends as with the same file without them
    one, _ = make_model(None, seed=3)
    build(one, data)
    two, _ = make_model(None, seed=4)
    build(two, data)
    assert checkpoint.load_state_dict(one, with_avg) == []
    assert checkpoint.load_state_dict(two, {k: v for k, v in with_avg.items() if not k.endswith(AVG)}) == []
    assert one.g_params.avg is None and two.g_params.avg is None and _same_model(one, two)
    assert torch.equal(one.g_params.flat, model.g_params.flat)


# ----------------------------------------------------------------------------------------------------------- 5: consumers
def _second_model_from_the_shadow(model, data):
    """A model without averaging whose LIVE generator weights are the first one's shadow."""
    from gansynth_amd import checkpoint
    state = checkpoint.state_dict(model)
    for name in model.g_params.named:
        state[name] = state.pop(name + AVG)
    second, _ = make_model(None, seed=7)
    build(second, data)
    checkpoint.load_state_dict(second, state)
    return second


def _mix_stand_in(waves, table, total, normalize=True, want_pcm=False):
    """The emulation backend has no mixdown: the fp32 statement of tests/synth_ref.py in its place (the same for both models compared)."""
    from tests import synth_ref as SRF
    out = torch.from_numpy(SRF.mix_f32(waves.numpy(), table, total))
    return out, None, out.abs().max().reshape(1)


def _score():
    from gansynth_amd.notes import Note
    return [Note(60, 100, 0.0, 0.004), Note(64, 80, 0.002, 0.008), Note(31, 127, 0.005, 0.009)]


SPECTRAL = dict(waveform_length=2 * 4 * 32, sample_rate=16000)


def test_consumers_read_the_average_and_leave_the_model_alone(cpu_backend, monkeypatch):
    from gansynth_amd import kernels, spectral_ops
    # (the reduced network's images are not 128 x 1024: the inverse transform is not what is under test here)
    monkeypatch.setattr(spectral_ops, "convert_images_to_waveform", lambda images, **kw: images.reshape(images.shape[0], -1).float())
    kernels.get().note_mix = _mix_stand_in
    model, data = make_model(0.999)
    train(model, 3)
    model.spectral_params = dict(SPECTRAL)
    second = _second_model_from_the_shadow(model, data)
    second.spectral_params = dict(SPECTRAL)
    assert torch.equal(second.g_params.flat, model.g_params.avg) and not torch.equal(model.g_params.flat, model.g_params.avg)
    flat, avg = model.g_params.flat.clone(), model.g_params.avg.clone()
    rng = torch.random.get_rng_state()
    lat, lab = data[1][0], data[1][1]
    kw = dict(normalize=False, batch_size=4, release_seconds=0.001, seconds_per_instrument=0.004, seed=2)
    want_wave, want_clip = use(second).generate(lat, lab), second.synthesize(_score(), **kw)
    wave = use(model).generate(lat, lab, weights="average")
    assert torch.equal(wave, want_wave) and not torch.equal(wave, model.generate(lat, lab))
    assert torch.equal(model.generate(lat, lab, weights="live"), model.generate(lat, lab))
    clip = model.synthesize(_score(), weights="average", **kw)
    assert torch.equal(clip, want_clip) and not torch.equal(clip, model.synthesize(_score(), **kw))
    assert torch.equal(model.g_params.flat, flat) and torch.equal(model.g_params.avg, avg)
    assert torch.equal(torch.random.get_rng_state(), rng) and not model._average_in
    with pytest.raises(ValueError, match="weights must be"):
        model.generate(lat, lab, weights="mean")
    # a following train_step equals the one of a model that never looked at its average
    never, _ = make_model(0.999)
    train(never, 3)
    a = train(model, 1)
    b = train(never, 1)
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][1], b[0][1])
    assert torch.equal(model.g_params.flat, never.g_params.flat) and torch.equal(model.g_params.avg, never.g_params.avg)
    assert torch.equal(model.d_params.flat, never.d_params.flat)


def test_no_average_to_read_is_an_error_that_names_the_key(cpu_backend, tmp_path, monkeypatch):
    from gansynth_amd import checkpoint, kernels, spectral_ops
    monkeypatch.setattr(spectral_ops, "convert_images_to_waveform", lambda images, **kw: images.reshape(images.shape[0], -1).float())
    kernels.get().note_mix = _mix_stand_in
    off, data = make_model(None)
    train(off, 1)
    off.spectral_params = dict(SPECTRAL)
    first = next(iter(off.g_params.named)) + AVG
    lat, lab = data[0][0], data[0][1]
    live = off.g_params.flat.clone()
    with pytest.raises(ValueError, match=first):                       # no shadow, no model_dir
        off.generate(lat, lab, weights="average")
    with pytest.raises(ValueError, match=first):
        off.synthesize(_score(), weights="average", batch_size=4, release_seconds=0.001)
    checkpoint.save(off, str(tmp_path / "off"))
    with pytest.raises(ValueError, match=first):                       # a checkpoint without averages
        off.synthesize(_score(), model_dir=str(tmp_path / "off"), weights="average", batch_size=4, release_seconds=0.001)
    with pytest.raises(ValueError, match=first):
        next(off.generate(model_dir=str(tmp_path / "off"), config=None, weights="average"))
    with pytest.raises(ValueError, match=first):                       # a directory without a checkpoint
        off.synthesize(_score(), model_dir=str(tmp_path / "empty"), weights="average", batch_size=4, release_seconds=0.001)
    assert off.g_params.avg is None and torch.equal(off.g_params.flat, live)
    # an inference-only model takes the averages from a checkpoint that has them
    on, _ = make_model(0.999)
    train(on, 2)
    on.spectral_params = dict(SPECTRAL)
    checkpoint.save(on, str(tmp_path / "on"))
    kw = dict(normalize=False, batch_size=4, release_seconds=0.001, seed=2)
    want_clip, want_wave = on.synthesize(_score(), weights="average", **kw), on.generate(data[0][0], data[0][1], weights="average")
    reader, _ = make_model(None, seed=5)
    reader.spectral_params = dict(SPECTRAL)
    clip = reader.synthesize(_score(), model_dir=str(tmp_path / "on"), weights="average", **kw)
    assert torch.equal(clip, want_clip)
    assert torch.equal(reader.g_params.avg, on.g_params.avg) and torch.equal(reader.g_params.flat, on.g_params.flat)
    batches = reader.generate(model_dir=str(tmp_path / "on"), config=None, weights="average")
    assert np.array_equal(next(batches), want_wave.numpy())
    assert not reader._average_in and torch.equal(reader.g_params.flat, on.g_params.flat)   # between two yields the model is as always


def test_nothing_trains_or_saves_while_the_average_is_swapped_in(cpu_backend, tmp_path):
    from gansynth_amd import checkpoint
    model, data = make_model(0.999)
    train(model, 2)
    flat, avg = model.g_params.flat.clone(), model.g_params.avg.clone()
    with model.averaged_generator():
        assert torch.equal(model.g_params.flat, avg) and torch.equal(model.g_params.avg, flat)
        for call in (model.train_step, lambda: model.discriminator_step(*data[0]), lambda: model.generator_step(data[0][0], data[0][1]),
                     lambda: checkpoint.state_dict(model), lambda: checkpoint.save(model, str(tmp_path))):
            with pytest.raises(RuntimeError, match="average is swapped in"):
                call()
    assert torch.equal(model.g_params.flat, flat) and torch.equal(model.g_params.avg, avg)
    assert not os.path.exists(str(tmp_path / "checkpoint"))
    with pytest.raises(KeyError):                                      # an exception raised inside still swaps back
        with model.averaged_generator():
            raise KeyError("from the body")
    assert torch.equal(model.g_params.flat, flat) and torch.equal(model.g_params.avg, avg) and not model._average_in
    train(model, 1)                                                    # and the model trains on


# ------------------------------------------------------------------------------------------------------------ 6: the decay
@pytest.mark.parametrize("decay", [1.0, -0.1, float("nan")])
def test_a_decay_outside_the_half_open_unit_interval_is_refused(cpu_backend, decay):
    with pytest.raises(ValueError, match="generator_average_decay"):
        make_model(decay)


def test_a_decay_of_zero_or_none_is_off(cpu_backend):
    for decay in (0, 0.0, None):
        model, data = make_model(decay)
        build(model, data)
        assert model.average_decay == 0.0 and model.g_params.avg is None and not model._averaging()


# --------------------------------------------------------------------------------------------------------------- 7: the ABI
def test_refusals_without_gpu():
    """Pure host-side checks (no kernel is launched): every refusal of include/gansynth_hip.h returns GS_ERR_ARG with a message."""
    from gansynth_amd import _lib
    lib = _lib.load()
    A, B, D = 0x10000, 0x20000, 0x30000   # (never dereferenced: the argument checks come first)
    pairs = [(lambda a, b, n: lib.gs_ema_step(a, b, n, 0.5, None), b"ema_step"),
             (lambda a, b, n: lib.gs_ema_step_dev(a, b, n, D, None), b"ema_step_dev"),
             (lambda a, b, n: lib.gs_swap_f32(a, b, n, None), b"swap_f32")]
    for call, name in pairs:
        for args, message in (((A, B, 0), b"numel"), ((A, B, -4), b"numel"), ((None, B, 64), b"null"), ((A, None, 64), b"null"),
                              ((A + 4, B, 64), b"16-byte"), ((A, B + 8, 64), b"16-byte"), ((A, A, 64), b"same"),
                              ((A, A + 64, 64), b"overlap")):
            assert call(*args) == -1, (name, args)
            err = lib.gs_last_error()
            assert name in err and message in err, (name, args, err)
    for om in (-0.1, 1.5, -1.0, float("nan"), float("inf")):
        assert lib.gs_ema_step(A, B, 64, om, None) == -1 and b"one_minus_decay" in lib.gs_last_error(), om
    assert lib.gs_ema_step_dev(A, B, 64, None, None) == -1 and b"one_minus_decay_dev" in lib.gs_last_error()
    # a decay of exactly 1 is no step: accepted, and nothing is launched (there is no device here to launch on)
    assert lib.gs_ema_step(A, B, 64, 0.0, None) == 0


# ------------------------------------------------------------------------------------------------------------ 8: the driver
def test_the_driver_lists_the_two_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "gan_synth_main.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "--generator_ema_decay" in out.stdout and "--weights {live,average}" in out.stdout
