"""Pitch-classifier driver on the MI355X path -- the command line of the reference's pitch_classifier_main.py (:23-31, :93-109).

    python pitch_classifier_main.py --train --model_dir pitch_classifier_model --filenames 'nsynth_train*.tfrecord'
    python pitch_classifier_main.py --evaluate --model_dir pitch_classifier_model --filenames 'nsynth_test*.tfrecord'

Same flags, defaults and hyper-parameters (:71-81: weight decay 1e-4, Nesterov momentum 0.9, learning rate 0.128 * batch / 256 decayed
by 0.1 every 70000 * epochs / 4 / batch steps).  `--synthetic` replaces `--filenames` by generated notes of the same shapes;
`--evaluate --synthetic` needs `--num_evaluate_batches` (one flag more than gan_synth_main.py's set: the generated input never ends).  The latest
checkpoint of `--model_dir` is also what `gan_synth_main.py --evaluate --classifier <file>` takes.  Training runs with fp32
activations; `--dtype` is the activation storage of `--evaluate`.  `--pack_bank PATH` packs `--filenames` into one file and exits (no
GPU needed); `--bank PATH` serves the same batches from that file, resident on the device (gansynth_amd/bank.py).
"""
import argparse
import glob

import torch

parser = argparse.ArgumentParser()
parser.add_argument("--model_dir", type=str, default="pitch_classifier_model")
parser.add_argument("--filenames", type=str, default="nsynth*.tfrecord")
parser.add_argument("--batch_size", type=int, default=64)
parser.add_argument("--num_epochs", type=int, default=100)
parser.add_argument("--total_steps", type=int, default=50000)
parser.add_argument("--train", action="store_true")
parser.add_argument("--evaluate", action="store_true")
# not in the reference
parser.add_argument("--synthetic", action="store_true", help="generated notes instead of --filenames")
parser.add_argument("--dtype", choices=["f32", "bf16"], default="f32", help="activation storage of --evaluate (training is fp32)")
parser.add_argument("--save_checkpoint_steps", type=int, default=1000)
parser.add_argument("--log_tensor_steps", type=int, default=100)
parser.add_argument("--save_summary_steps", type=int, default=100, help="TensorBoard summaries into --model_dir every this many steps (0: off)")
parser.add_argument("--pack_bank", type=str, default=None, metavar="PATH",
                    help="pack the notes of --filenames (pitches 24-84, acoustic sources) into PATH and exit; needs no GPU")
parser.add_argument("--bank", type=str, default=None, metavar="PATH",
                    help="serve --train / --evaluate from the packed notes of PATH, resident on the device, instead of --filenames")
parser.add_argument("--num_evaluate_batches", type=int, default=None, help="stop --evaluate --synthetic after this many batches (synthetic input never ends)")


def hyper_params(batch_size, num_epochs):
    """pitch_classifier_main.py:71-81."""
    from gansynth_amd.models import exponential_decay
    from gansynth_amd.utils import Dict
    return Dict(weight_decay=1e-4,
                learning_rate=lambda global_step: exponential_decay(0.128 * batch_size / 256, global_step,
                                                                    decay_steps=70000 * num_epochs / 4 / batch_size, decay_rate=0.1),
                momentum=0.9, use_nesterov=True)


def main(args):
    if args.pack_bank is not None:   # host work only, before any device is touched
        from gansynth_amd import bank
        files = sorted(glob.glob(args.filenames))
        if not files:
            raise SystemExit(f"--pack_bank: --filenames {args.filenames} matches no file")
        header = bank.pack(files, args.pack_bank, pitches=range(24, 85), sources=[0])
        print(f"{header['rows']} of {header['total_records']} notes packed into {args.pack_bank}")
        return
    torch.cuda.set_device(0)
    from gansynth_amd import variables
    from gansynth_amd.bank import NoteBank, bank_input_fn
    from gansynth_amd.dataset import nsynth_input_fn, synthetic_nsynth_input_fn
    from gansynth_amd.models import PitchClassifier
    from gansynth_amd.networks import ResNet
    from gansynth_amd.utils import Dict

    torch.manual_seed(0)   # tf.set_random_seed(0) (:37)
    device = torch.device("cuda", 0)
    pitches = range(24, 85)
    banks = {}   # (--train and --evaluate in one run share one upload)

    def input_fn_factory(train):
        if args.synthetic:
            if not train and args.num_evaluate_batches is None:
                raise SystemExit("--evaluate --synthetic needs --num_evaluate_batches (synthetic input never ends)")
            return synthetic_nsynth_input_fn(args.batch_size, pitches, device=device, seed=0, num_batches=None if train else args.num_evaluate_batches)
        if args.bank is not None:
            if "open" not in banks:
                banks["open"] = NoteBank.open(args.bank)
            return bank_input_fn(banks["open"], args.batch_size, args.num_epochs if train else 1, shuffle=train, pitches=pitches,
                                 sources=[0], device=device, seed=0)
        return nsynth_input_fn(sorted(glob.glob(args.filenames)), args.batch_size, args.num_epochs if train else 1, shuffle=train,
                               pitches=pitches, sources=[0], device=device, seed=0)

    resnet = ResNet.pitch_classifier(store=variables.VariableStore(device="cuda", seed=0))   # :39-50
    spectral = Dict(waveform_length=64000, sample_rate=16000, spectrogram_shape=[128, 1024], overlap=0.75)

    if args.train:
        classifier = PitchClassifier(resnet, input_fn_factory(True), spectral, hyper_params(args.batch_size, args.num_epochs))
        classifier.train(                              # pitch_classifier_main.py:95-102, argument for argument
            model_dir=args.model_dir,
            config=None,                               # (the reference's tf.ConfigProto: nothing of it applies here)
            total_steps=args.total_steps,
            save_checkpoint_steps=args.save_checkpoint_steps,
            save_summary_steps=args.save_summary_steps,
            log_tensor_steps=args.log_tensor_steps)
        print(f"stopped at global_step = {classifier.global_step}")

    if args.evaluate:
        classifier = PitchClassifier(resnet, input_fn_factory(False), spectral, hyper_params(args.batch_size, args.num_epochs),
                                     dtype=torch.float32 if args.dtype == "f32" else torch.bfloat16)
        print(classifier.evaluate(model_dir=args.model_dir, config=None))


if __name__ == "__main__":
    main(parser.parse_args())
