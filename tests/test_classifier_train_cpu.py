"""CPU: the host side of the pitch classifier's training -- learning-rate schedule, the decayed-variable partition, the checkpoint
name space, the command line of pitch_classifier_main.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exponential_decay_closed_form():
    from gansynth_amd.models import exponential_decay
    assert exponential_decay(0.032, 0, 27343.75, 0.1) == 0.032
    assert exponential_decay(0.032, 27343.75, 27343.75, 0.1) == pytest.approx(0.0032, rel=1e-12)
    assert exponential_decay(0.032, 13671.875, 27343.75, 0.1) == pytest.approx(0.032 * 0.1 ** 0.5, rel=1e-12)   # not a staircase
    assert exponential_decay(1.0, 3, 2, 0.25) == pytest.approx(0.125, rel=1e-12)


def test_reference_hyper_parameters():
    sys.path.insert(0, ROOT)
    try:
        import pitch_classifier_main as M
    finally:
        sys.path.remove(ROOT)
    hp = M.hyper_params(64, 100)
    assert hp.weight_decay == 1e-4 and hp.momentum == 0.9 and hp.use_nesterov is True
    assert hp.learning_rate(0) == pytest.approx(0.128 * 64 / 256)
    assert hp.learning_rate(70000 * 100 / 4 / 64) == pytest.approx(0.128 * 64 / 256 * 0.1)


def test_parser_has_the_reference_flags_and_defaults():
    sys.path.insert(0, ROOT)
    try:
        import pitch_classifier_main as M
    finally:
        sys.path.remove(ROOT)
    args = M.parser.parse_args([])
    assert (args.model_dir, args.filenames, args.batch_size, args.num_epochs, args.total_steps, args.train, args.evaluate) == \
        ("pitch_classifier_model", "nsynth*.tfrecord", 64, 100, 50000, False, False)
    assert (args.synthetic, args.dtype, args.save_checkpoint_steps, args.log_tensor_steps) == (False, "f32", 1000, 100)
    args = M.parser.parse_args(["--train", "--evaluate", "--synthetic", "--total_steps", "7"])
    assert args.train and args.evaluate and args.synthetic and args.total_steps == 7


def _cpu_net():
    from gansynth_amd import variables
    from gansynth_amd.networks import ResNet
    return ResNet.pitch_classifier(store=variables.VariableStore(device="cpu"))


def test_decayed_partition_of_the_full_classifier():
    from gansynth_amd.networks import ResNet
    names = list(_cpu_net().create_variables())
    decayed = [k for k in names if ResNet.is_decayed(k)]
    kept = [k for k in names if not ResNet.is_decayed(k)]
    assert len(names) == 16 * 8 + 4 + 2 + 2 + 2                     # 16 blocks x (2 norms x 2 + 2 convs x 2), 4 projections, stem, head norm, logits
    assert all(k.endswith("/gamma") or k.endswith("/beta") for k in kept) and len(kept) == 2 * (2 * 16 + 1)
    assert not any("normalization" in k for k in decayed)
    for k in ("resnet/conv/weight", "resnet/conv/bias", "resnet/logits/weight", "resnet/logits/bias",
              "resnet/residual_block_1_0/projection_shortcut/weight", "resnet/residual_block_3_2/conv_2nd/bias"):
        assert k in decayed, k
    assert "resnet/group_normalization/gamma" in kept and "resnet/residual_block_0_0/group_normalization_1st/beta" in kept


def test_checkpoint_name_space_round_trip(tmp_path):
    """Slots and the step never start with "resnet/": a checkpoint passes ResNet.load_state_dict(strict=True) as a weight file."""
    from tests import resnet_ref as RR
    from gansynth_amd import classifier_io
    from gansynth_amd.models import PitchClassifier
    net = _cpu_net()
    shapes = [(k, tuple(v.shape)) for k, v in net.create_variables().items()]
    small = [ks for ks in shapes if int(np.prod(ks[1])) <= 4096]   # (the name space, not the 85 MB of weights)
    weights = RR.random_params(small, seed=1)
    state = dict(weights)
    for k, v in weights.items():
        state[PitchClassifier.slot_name(k)] = 0.5 * v
    state["global_step"] = np.asarray(2 ** 24 + 1, dtype=np.int64)   # (an integer entry: exact past float32's 2^24)
    assert not any(k.startswith("resnet/") for k in state if k not in weights)
    path = str(tmp_path / "model.ckpt-16777217.safetensors")
    classifier_io.write_safetensors(path, state)
    back = classifier_io.read_safetensors(path)
    w2, slots, step = PitchClassifier.split_state(back)
    assert step == 2 ** 24 + 1 and back["global_step"].dtype == np.int64 and sorted(w2) == sorted(weights) and sorted(slots) == sorted(weights)
    for k in weights:
        assert np.array_equal(w2[k], weights[k]) and np.array_equal(slots[k], 0.5 * weights[k])
    # strict=True refuses unknown "resnet/..." entries only: the slots pass, the missing large variables are named
    with pytest.raises(KeyError, match="lack the variable"):
        net.load_state_dict(back, strict=True)
    full = {k: np.zeros(s, dtype=np.float32) for k, s in shapes if k not in weights}
    net.load_state_dict({**back, **full}, strict=True)
    assert np.array_equal(net.store.variables["resnet/conv/bias"].detach().numpy(), weights["resnet/conv/bias"])
    with pytest.raises(KeyError, match="does not have"):
        net.load_state_dict({**back, **full, "resnet/extra": np.zeros(1)}, strict=True)
