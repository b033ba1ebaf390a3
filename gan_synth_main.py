"""GANSynth driver on the MI355X path -- the command line of the reference's gan_synth_main.py (:26-37, :102-139).

    python gan_synth_main.py --train --model_dir gan_synth_model --filenames 'nsynth*.tfrecord' --batch_size 8 \
        --total_steps 1000000 --growing_steps 1000000
    python gan_synth_main.py --generate --model_dir gan_synth_model --filenames 'nsynth_test*.tfrecord'

Same flags and defaults; `--filenames` takes the reference's tfrecord files (or NSynth `examples.json` indexes) and
`--synthetic` replaces them by generated notes of the same shapes when no dataset is at hand.  Multi-GPU: launch with
`python -m torch.distributed.run --nproc-per-node N gan_synth_main.py ...` (one process per GPU, gradients all-reduced over
RCCL; the learning rates scale with the global batch like :79,82).  `--evaluate` prints the Frechet distance between the pitch
classifier's features of real and generated notes (:111-124); `--classifier` names the reference's frozen classifier graph (a
TensorFlow GraphDef, read without TensorFlow) or the same weights as a .safetensors file:

    python gan_synth_main.py --evaluate --model_dir gan_synth_model --filenames 'nsynth_test*.tfrecord' --classifier pitch_classifier.pb

`--ndb` (not in the reference's driver) adds the other figures of its metrics.py to that dict: inception_score, pitch_accuracy,
num_different_bins and bin_jsd, the k-means of NDB on HIP kernels (gansynth_amd/kmeans.py, DESIGN.md "NDB on the device"):

    python gan_synth_main.py --evaluate --ndb --model_dir gan_synth_model --filenames 'nsynth_test*.tfrecord' --classifier pitch_classifier.pb

`--swd` (not in the reference's driver) adds sliced_wasserstein_distance and sliced_wasserstein_distance_levels, the metric of the
progressive-GAN paper on HIP kernels (gansynth_amd/swd.py, DESIGN.md "SWD on the device"); it needs no classifier, and with
`--classifier none` none is loaded and these are the only figures:

    python gan_synth_main.py --evaluate --swd --model_dir gan_synth_model --filenames 'nsynth_test*.tfrecord' --classifier pitch_classifier.pb
    python gan_synth_main.py --evaluate --swd --classifier none --model_dir gan_synth_model --filenames 'nsynth_test*.tfrecord'

`--prd` (not in the reference's driver) adds precision, recall, density and coverage of the generated features against the real ones, which
tell a generator that makes bad notes (precision, density) from one that makes too few kinds (recall, coverage); `--prd_k` is the neighbour
that sets a row's radius (default 3).  k-nearest-neighbour radii on HIP kernels (gansynth_amd/manifold.py, DESIGN.md "Precision and recall on
the device"); the figures come from the classifier's features, so `--classifier none` is refused:

    python gan_synth_main.py --evaluate --prd --model_dir gan_synth_model --filenames 'nsynth_test*.tfrecord' --classifier pitch_classifier.pb
    python gan_synth_main.py --evaluate --ndb --prd --prd_k 5 --model_dir gan_synth_model --filenames 'nsynth_test*.tfrecord' --classifier pitch_classifier.pb

`--f0` (not in the reference's driver) measures pitch on the AUDIO, without a classifier: a YIN f0 tracker on HIP kernels (gansynth_amd/pitch.py,
DESIGN.md "Pitch tracking on the device") follows every real and every generated note, and the dict gains f0_pitch_accuracy (the share of notes
within 50 cents of their label), f0_chroma_accuracy (the same up to octaves), f0_median_abs_cents, f0_jitter_cents and f0_voiced_fraction for the
generated notes and the same five with the prefix real_ -- the calibration to read them against, since YIN is not perfect on real instruments.
It needs no classifier either:

    python gan_synth_main.py --evaluate --f0 --model_dir gan_synth_model --filenames 'nsynth_test*.tfrecord' --classifier pitch_classifier.pb
    python gan_synth_main.py --evaluate --f0 --classifier none --model_dir gan_synth_model --filenames 'nsynth_test*.tfrecord'

`--kid` (not in the reference's driver) adds the kernel inception distance (Binkowski et al. 2018) of the generated features against the real
ones: kernel_inception_distance, the unbiased estimate of the squared maximum mean discrepancy under the cubic kernel over all notes -- unlike
the Frechet distance its expectation does not depend on the number of notes, and it may be negative -- and kernel_inception_distance_subset_mean
and kernel_inception_distance_subset_std over `--kid_subsets` seeded subsets (default 100) of `--kid_subset_size` notes a side (default 1000, or
all there are).  All pairs on an fp64 matrix-core HIP kernel (gansynth_amd/kid.py, DESIGN.md "KID on the device"); the figures come from the
classifier's features, so `--classifier none` is refused:

    python gan_synth_main.py --evaluate --kid --model_dir gan_synth_model --filenames 'nsynth_test*.tfrecord' --classifier pitch_classifier.pb
    python gan_synth_main.py --evaluate --prd --kid --kid_subsets 50 --kid_subset_size 500 --model_dir gan_synth_model --filenames 'nsynth_test*.tfrecord' --classifier pitch_classifier.pb

`--synthesize` (not in the reference) renders a score -- a Standard MIDI File or a JSON list of {"pitch", "velocity", "start", "end"}
notes -- into one 16 kHz 16-bit WAV: every note generated at its pitch, the timbre gliding between latent anchors, the mixdown on the
device (GANSynth.synthesize).  It needs no dataset:

    python gan_synth_main.py --synthesize score.mid --model_dir gan_synth_model --output score.wav

`--ensemble` gives every part of the score -- a MIDI channel under one program, a JSON "part" -- its own instrument and honours the channel
volume; `--stereo` writes two channels placed by pan (CC 10, JSON "pan") and, for the parts without one, fanned out by `--spread` in [0, 1];
both channels are normalised by ONE peak (GANSynth.synthesize with ensemble / stereo / spread, DESIGN.md "Parts and stereo"):

    python gan_synth_main.py --synthesize quartet.mid --ensemble --stereo --spread 0.6 --output quartet.wav

`--output_rate HZ` (not in the reference; default: the model's 16000) writes the files of `--synthesize` and `--generate` at another
sample rate, e.g. 44100 or 48000: resampled on the device, and for `--synthesize` peak-normalised and quantised THERE (GANSynth.synthesize
with sample_rate, DESIGN.md "Output rates").

`--reverb SECONDS` (not in the reference) puts the rendered score into a designed room of that RT60, `--reverb_ir FILE.wav` into a recorded
one (a mono or stereo impulse response; the two exclude each other); `--reverb_mix W` in [0, 1] is the share of the reverberated signal
(default 0.25) and `--reverb_predelay SECONDS` delays it (default 0).  The stage runs on the device at the output rate, between the
resampler and the ONE peak normalisation, and the file grows by the tail (gansynth_amd/reverb.py, DESIGN.md "Reverb"):

    python gan_synth_main.py --synthesize quartet.mid --ensemble --stereo --output_rate 48000 --reverb 1.8 --reverb_mix 0.3 --output quartet.wav

`--limit DB` (not in the reference) ends the chain of `--synthesize` with a look-ahead limiter instead of the division by the peak: the
clip is scaled so that its peak would stand `--limit_drive DB` (default 6) above the ceiling of DB dBFS (<= 0), and a smooth gain, looking
`--limit_lookahead SECONDS` ahead (default 0.005), pulls back only the peaks; no sample of the file exceeds the ceiling
(gansynth_amd/limiter.py, DESIGN.md "Limiter"):

    python gan_synth_main.py --synthesize quartet.mid --ensemble --stereo --output_rate 48000 --reverb 1.8 --limit -1 --limit_drive 9 --output quartet.wav

`--loudness LUFS` (not in the reference) ends the chain of `--synthesize` at a target programme loudness instead of a peak level: the
clip is measured (ITU-R BS.1770-4 integrated loudness, the K-weighted energies on the device), scaled to the target, and the limiter holds
the peaks under `--limit DB` (default -1 dBFS) looking `--limit_lookahead` ahead; `--limit_drive` does not apply, the level is set by the
target (gansynth_amd/loudness.py, DESIGN.md "Loudness"):

    python gan_synth_main.py --synthesize quartet.mid --ensemble --stereo --output_rate 48000 --reverb 1.8 --loudness -16 --output quartet.wav

`--true_peak` (not in the reference) reads the ceiling of `--limit` -- alone or under `--loudness` -- in dBTP: the peak of the reconstructed
waveform, measured on the 4x oversampled signal (ITU-R BS.1770-4 Annex 2; EBU R128 asks for -1 dBTP), which a file limited by its samples
alone exceeds by 2-3 dB.  The limiter then follows the detector's envelope, and the summary states the file's true peak
(gansynth_amd/true_peak.py, DESIGN.md "True peak"):

    python gan_synth_main.py --synthesize quartet.mid --ensemble --stereo --output_rate 48000 --reverb 1.8 --loudness -16 --limit -1 --true_peak --output quartet.wav

`--controllers` honours what a score says after a note has started (GANSynth.synthesize with controllers, DESIGN.md "Controllers"): channel
volume (CC 7) and expression (CC 11) as they move, pan (CC 10) with `--stereo`, and the sustain pedal (CC 64), which holds notes past their
key-up; every change takes effect over `--controller_ramp` seconds (default 0.01):

    python gan_synth_main.py --synthesize sonata.mid --controllers --output sonata.wav
    python gan_synth_main.py --synthesize quartet.mid --ensemble --stereo --controllers --controller_ramp 0.02 --output quartet.wav

`--bend` honours pitch bend (GANSynth.synthesize with bend, DESIGN.md "Pitch bend"): the wheel's messages and the range set through RPN 0,0
become one playback-rate curve per part, and the notes it touches are resampled along it on the device before the mix; the clip's length
and every onset stay as they are.  A change takes effect over `--controller_ramp` seconds, which `--bend` shares with `--controllers`:

    python gan_synth_main.py --synthesize lead.mid --bend --output lead.wav
    python gan_synth_main.py --synthesize quartet.mid --ensemble --stereo --controllers --bend --controller_ramp 0.005 --output quartet.wav

`--sustain` holds notes past the four seconds the generator makes (GANSynth.synthesize with sustain, DESIGN.md "Sustain"): a note the score
holds longer -- an organ chord, a tied whole note, a pedalled piano with `--controllers` -- is looped on the device at a length found by
correlation and keeps its whole release, and the clip is as long as the score says.  A held note that `--bend` bends is cut as before:

    python gan_synth_main.py --synthesize organ.mid --sustain --output organ.wav

`--pack_bank` / `--bank` (not in the reference): the notes packed once into one file (on any machine, no GPU needed), then held on the
device and drawn there, batch for batch what `--filenames` yields (gansynth_amd/bank.py, DESIGN.md "Resident notes"):

    python gan_synth_main.py --pack_bank nsynth_train.bank --filenames 'nsynth_train*.tfrecord'
    python gan_synth_main.py --train --model_dir gan_synth_model --bank nsynth_train.bank
"""
import argparse
import glob
import math
import os

import torch

parser = argparse.ArgumentParser()
parser.add_argument("--model_dir", type=str, default="gan_synth_model")
parser.add_argument("--filenames", type=str, default="nsynth*.tfrecord")
parser.add_argument("--batch_size", type=int, default=8)
parser.add_argument("--num_epochs", type=int, default=None)
parser.add_argument("--total_steps", type=int, default=1000000)
parser.add_argument("--growing_steps", type=int, default=1000000)
parser.add_argument("--classifier", type=str, default="pitch_classifier.pb")
parser.add_argument("--train", action="store_true")
parser.add_argument("--evaluate", action="store_true")
parser.add_argument("--generate", action="store_true")
# not in the reference
parser.add_argument("--synthetic", action="store_true", help="generated notes instead of --filenames")
parser.add_argument("--ndb", action="store_true",
                    help="--evaluate: also the inception score, the pitch accuracy and the number of statistically different bins (NDB) with the "
                         "Jensen-Shannon divergence of the bin proportions, the k-means on the device (no scikit-learn)")
parser.add_argument("--swd", action="store_true",
                    help="--evaluate: also the sliced Wasserstein distance between Laplacian-pyramid patches of the real and generated images, one "
                         "figure a pyramid level and their mean, on the device; with --classifier none these are the only figures")
parser.add_argument("--prd", action="store_true",
                    help="--evaluate: also precision, recall, density and coverage of the generated features against the real ones, from "
                         "k-nearest-neighbour radii on the device; needs the classifier")
parser.add_argument("--f0", action="store_true",
                    help="--evaluate: also the pitch accuracy of the audio itself, real and generated, from a YIN f0 tracker on the device: accuracy within "
                         "50 cents, the same up to octaves, median deviation, jitter and voiced fraction; needs no classifier")
parser.add_argument("--prd_k", type=int, default=3, help="--prd: the neighbour whose distance is a row's radius")
parser.add_argument("--kid", action="store_true",
                    help="--evaluate: also the kernel inception distance of the generated features against the real ones, over all notes and as mean "
                         "and standard deviation over subsets, all pairs on the device in fp64; needs the classifier")
parser.add_argument("--kid_subsets", type=int, default=100, help="--kid: the number of subsets behind the mean and the standard deviation (0: none)")
parser.add_argument("--kid_subset_size", type=int, default=1000, help="--kid: notes a side of a subset (at most all there are)")
parser.add_argument("--dtype", choices=["f32", "bf16"], default="bf16", help="activation storage (master weights / Adam stay fp32)")
parser.add_argument("--save_checkpoint_steps", type=int, default=1000)
parser.add_argument("--log_tensor_steps", type=int, default=100)
parser.add_argument("--save_summary_steps", type=int, default=100, help="TensorBoard summaries into --model_dir every this many steps (0: off)")
parser.add_argument("--num_generate_batches", type=int, default=None, help="stop --generate after this many batches (synthetic input never ends)")
parser.add_argument("--synthesize", type=str, default=None, metavar="PATH", help="render a score (.mid, .midi or .json) into --output")
parser.add_argument("--output", type=str, default="synthesized.wav", help="the WAV file --synthesize writes")
parser.add_argument("--seconds_per_instrument", type=float, default=6.0, help="--synthesize: seconds between two latent anchors")
parser.add_argument("--release_seconds", type=float, default=1.0, help="--synthesize: length of a note's linear release")
parser.add_argument("--output_rate", type=int, default=None, metavar="HZ",
                    help="--synthesize, --generate: the sample rate of the files written (default: the model's rate), resampled on the device")
parser.add_argument("--seed", type=int, default=0, help="--synthesize: seed of the latent anchors (a generator of their own)")
parser.add_argument("--ensemble", action="store_true",
                    help="--synthesize: every part of the score (a MIDI channel under one program, a JSON \"part\") plays its own instrument, "
                         "and the channel volume (CC 7) enters the gain")
parser.add_argument("--stereo", action="store_true",
                    help="--synthesize: a two-channel WAV: pan (CC 10, JSON \"pan\") and --spread place the notes, both channels share one peak")
parser.add_argument("--spread", type=float, default=0.0, metavar="FLOAT",
                    help="--synthesize --stereo: how far the parts without a pan fan out between left and right (0: all in the centre .. 1)")
parser.add_argument("--controllers", action="store_true",
                    help="--synthesize: honour what the score says after a note has started: channel volume (CC 7), expression (CC 11), "
                         "pan (CC 10, with --stereo) and the sustain pedal (CC 64), as one gain curve per part")
parser.add_argument("--controller_ramp", type=float, default=0.01, metavar="SECONDS",
                    help="--controllers, --bend: the length of the linear ramp with which a controller or bend change takes effect")
parser.add_argument("--bend", action="store_true",
                    help="--synthesize: honour pitch bend (and the range set through RPN 0,0): the notes it touches are resampled along "
                         "their part's bend curve on the device before the mix")
parser.add_argument("--sustain", action="store_true",
                    help="--synthesize: hold notes past the generated four seconds: a note the score holds longer is looped on the device "
                         "and keeps its whole release")
parser.add_argument("--reverb", type=float, default=None, metavar="SECONDS",
                    help="--synthesize: reverberate the clip in a designed room with this RT60 (seeded by --seed; two channels with --stereo)")
parser.add_argument("--reverb_ir", type=str, default=None, metavar="FILE.wav",
                    help="--synthesize: reverberate the clip with this recorded impulse response (mono or stereo WAV) instead of --reverb")
parser.add_argument("--reverb_mix", type=float, default=0.25, metavar="W",
                    help="--reverb, --reverb_ir: the share of the reverberated signal in [0, 1]; the dry clip keeps 1 - W")
parser.add_argument("--reverb_predelay", type=float, default=0.0, metavar="SECONDS", help="--reverb, --reverb_ir: silence in front of the room's response")
parser.add_argument("--limit", type=float, default=None, metavar="DB",
                    help="--synthesize: end with a look-ahead limiter at this ceiling in dBFS (<= 0) instead of the division by the peak")
parser.add_argument("--limit_drive", type=float, default=6.0, metavar="DB",
                    help="--limit: how far above the ceiling the clip's peak is driven before the limiter brings it back (>= 0; 0: peak normalisation)")
parser.add_argument("--limit_lookahead", type=float, default=0.005, metavar="SECONDS", help="--limit: the limiter's look-ahead (attack and release)")
parser.add_argument("--true_peak", action="store_true",
                    help="--limit / --loudness: read the ceiling in dBTP -- the limiter holds the 4x oversampled (reconstructed) waveform under it")
parser.add_argument("--loudness", type=float, default=None, metavar="LUFS",
                    help="--synthesize: end at this integrated loudness (BS.1770, <= 0 LUFS); the limiter holds the peaks under --limit (default -1 dBFS)")
parser.add_argument("--generator_ema_decay", type=float, default=0.0,
                    help="keep an exponential moving average of the generator's weights with this decay (0.0: off; progressive GAN uses 0.999)")
parser.add_argument("--pack_bank", type=str, default=None, metavar="PATH",
                    help="pack the notes of --filenames (pitches 24-84, acoustic sources) into PATH and exit; needs no GPU")
parser.add_argument("--bank", type=str, default=None, metavar="PATH",
                    help="serve --train / --evaluate / --generate from the packed notes of PATH, resident on the device, instead of --filenames")
parser.add_argument("--weights", choices=["live", "average"], default="live",
                    help="--generate, --evaluate, --synthesize: the generator's weights as trained, or their moving average "
                         "(from --generator_ema_decay of this run, or from the checkpoint's averages)")


def check_reverb_args(args):
    """The four reverb flags against each other and against --synthesize: SystemExit with a message.  -> whether a reverb is asked for."""
    room, recorded = getattr(args, "reverb", None), getattr(args, "reverb_ir", None)
    mix, predelay = getattr(args, "reverb_mix", 0.25), getattr(args, "reverb_predelay", 0.0)
    if room is not None and recorded is not None:
        raise SystemExit("--reverb (a designed room) and --reverb_ir (a recorded one) exclude each other")
    wanted = room is not None or recorded is not None
    if not wanted and (mix != 0.25 or predelay != 0.0):
        raise SystemExit("--reverb_mix and --reverb_predelay need --reverb or --reverb_ir")
    if wanted and args.synthesize is None:
        raise SystemExit("--reverb and --reverb_ir apply to --synthesize only")
    if room is not None and not room > 0:
        raise SystemExit(f"--reverb takes a positive RT60 in seconds (got {room})")
    if wanted and not 0.0 <= mix <= 1.0:
        raise SystemExit(f"--reverb_mix must be in [0, 1] (got {mix})")
    if wanted and not predelay >= 0:
        raise SystemExit(f"--reverb_predelay must not be negative (got {predelay})")
    return wanted


def check_limit_args(args):
    """The three limiter flags against each other and against --synthesize: SystemExit with a message.  -> whether a limiter is asked for."""
    ceiling = getattr(args, "limit", None)
    drive, lookahead = getattr(args, "limit_drive", 6.0), getattr(args, "limit_lookahead", 0.005)
    wanted = ceiling is not None
    if not wanted and (drive != 6.0 or lookahead != 0.005) and getattr(args, "loudness", None) is None:   # (--loudness has a limiter of its own)
        raise SystemExit("--limit_drive and --limit_lookahead need --limit")
    if wanted and args.synthesize is None:
        raise SystemExit("--limit applies to --synthesize only")
    if wanted and not ceiling <= 0:
        raise SystemExit(f"--limit takes a ceiling in dBFS, at most 0 (got {ceiling})")
    if wanted and not 0 <= drive < float("inf"):
        raise SystemExit(f"--limit_drive must be a non-negative number of dB (got {drive})")
    if wanted and not 0 <= lookahead < float("inf"):
        raise SystemExit(f"--limit_lookahead must be a non-negative number of seconds (got {lookahead})")
    if wanted and ceiling == float("-inf"):
        raise SystemExit(f"--limit takes a finite ceiling in dBFS (got {ceiling})")
    return wanted


def check_loudness_args(args):
    """--loudness against --synthesize and the limiter's flags: SystemExit with a message.  -> whether a loudness target is asked for."""
    target = getattr(args, "loudness", None)
    if target is None:
        return False
    if not math.isfinite(target):
        raise SystemExit(f"--loudness takes a finite target in LUFS (got {target})")
    if target > 0:
        raise SystemExit(f"--loudness takes a target in LUFS, at most 0 (got {target})")
    if args.synthesize is None:
        raise SystemExit("--loudness applies to --synthesize only")
    if getattr(args, "limit_drive", 6.0) != 6.0:
        raise SystemExit("--limit_drive does not apply with --loudness: the level is set by --loudness")
    lookahead = getattr(args, "limit_lookahead", 0.005)
    if not 0 <= lookahead < float("inf"):   # (check_limit_args looks at it only with --limit)
        raise SystemExit(f"--limit_lookahead must be a non-negative number of seconds (got {lookahead})")
    return True


def check_true_peak_args(args):
    """--true_peak against --limit / --loudness: SystemExit with a message.  -> whether the ceiling is read in dBTP."""
    if not getattr(args, "true_peak", False):
        return False
    if getattr(args, "limit", None) is None and getattr(args, "loudness", None) is None:
        raise SystemExit("--true_peak needs --limit or --loudness: it says how their ceiling is read")
    return True


def check_controller_args(args):
    """--controllers, --controller_ramp, --bend and --sustain against each other and against --synthesize: SystemExit with a message.
    -> whether controllers are asked for."""
    wanted, ramp = getattr(args, "controllers", False), getattr(args, "controller_ramp", 0.01)
    bend = getattr(args, "bend", False)   # (--bend shares the ramp)
    if not wanted and not bend and ramp != 0.01:   # (NaN differs from everything)
        raise SystemExit("--controller_ramp needs --controllers")
    if wanted and args.synthesize is None:
        raise SystemExit("--controllers applies to --synthesize only")
    if bend and args.synthesize is None:
        raise SystemExit("--bend applies to --synthesize only")
    if getattr(args, "sustain", False) and args.synthesize is None:
        raise SystemExit("--sustain applies to --synthesize only")
    if (wanted or bend) and not 0 <= ramp < float("inf"):
        raise SystemExit(f"--controller_ramp must be a finite, non-negative number of seconds (got {ramp})")
    return wanted


def check_prd_args(args):
    """--prd and --prd_k against --evaluate and --classifier: SystemExit with a message.  -> whether the four figures are asked for."""
    wanted, k = getattr(args, "prd", False), getattr(args, "prd_k", 3)
    if not wanted and k != 3:
        raise SystemExit("--prd_k needs --prd")
    if wanted and not getattr(args, "evaluate", False):
        raise SystemExit("--prd applies to --evaluate only")
    if wanted and str(getattr(args, "classifier", "")).lower() == "none":
        raise SystemExit("--prd needs the pitch classifier (precision, recall, density and coverage come from its features): not --classifier none")
    if wanted and not 1 <= k <= 8:
        raise SystemExit(f"--prd_k must be in [1, 8] (got {k})")
    return wanted


def check_kid_args(args):
    """--kid, --kid_subsets and --kid_subset_size against --evaluate and --classifier: SystemExit with a message.  -> whether the figures are asked for."""
    wanted, subsets, size = getattr(args, "kid", False), getattr(args, "kid_subsets", 100), getattr(args, "kid_subset_size", 1000)
    if not wanted and (subsets != 100 or size != 1000):
        raise SystemExit("--kid_subsets and --kid_subset_size need --kid")
    if wanted and not getattr(args, "evaluate", False):
        raise SystemExit("--kid applies to --evaluate only")
    if wanted and str(getattr(args, "classifier", "")).lower() == "none":
        raise SystemExit("--kid needs the pitch classifier (the kernel inception distance comes from its features): not --classifier none")
    if wanted and subsets < 0:
        raise SystemExit(f"--kid_subsets must not be negative (got {subsets})")
    if wanted and size < 2:
        raise SystemExit(f"--kid_subset_size must be at least 2 (got {size})")
    return wanted


def synthesize_to_wav(model, args, pitches, restore=True, log=print):
    """--synthesize: the score args.synthesize through GANSynth.synthesize into the 16-bit WAV args.output (the kernel's own PCM: [T], or
    the interleaved [T, 2] of --stereo, which is a two-channel WAV's layout).  With --reverb / --reverb_ir: the unnormalised clip at the
    output rate, then reverb.apply -- the room, ONE peak and the PCM there.  With --limit: whichever stage comes last hands over its
    unnormalised clip and its peak, and limiter.apply writes the PCM.  With --loudness: the same hand-over, and loudness.apply -- measure, scale to
    the target, limit at the ceiling of --limit (or -1 dBFS) -- writes the PCM."""
    from scipy.io import wavfile
    from gansynth_amd import checkpoint
    reverb_wanted = check_reverb_args(args)
    limit_wanted = check_limit_args(args)
    loudness_wanted = check_loudness_args(args)
    controllers_wanted = check_controller_args(args)
    true_peak_wanted = check_true_peak_args(args)
    extra = dict(true_peak=True) if true_peak_wanted else {}   # (without the flag the calls are the ones they were)
    last_wanted = limit_wanted or loudness_wanted   # a stage after the reverb that sets the level and quantises
    if os.path.splitext(args.synthesize)[1].lower() not in (".mid", ".midi", ".json"):
        raise SystemExit(f"--synthesize takes a .mid, .midi or .json score (got {args.synthesize})")
    if restore and checkpoint.latest(args.model_dir) is None:
        log("no checkpoint found: synthesizing from the initial weights")
        restore = False
    info = {}
    how = dict(model_dir=args.model_dir if restore else None, seed=args.seed, seconds_per_instrument=args.seconds_per_instrument,
               release_seconds=args.release_seconds, info=info, pitches=pitches, batch_size=args.batch_size, weights=args.weights,
               sample_rate=getattr(args, "output_rate", None), ensemble=getattr(args, "ensemble", False),
               stereo=getattr(args, "stereo", False), spread=getattr(args, "spread", 0.0))
    if controllers_wanted:   # (without the flag the call is the one it was)
        how.update(controllers=True, controller_ramp=args.controller_ramp)
    bend_wanted = getattr(args, "bend", False)
    if bend_wanted:
        how.update(bend=True, controller_ramp=args.controller_ramp)
    sustain_wanted = getattr(args, "sustain", False)
    if sustain_wanted:
        how.update(sustain=True)
    if reverb_wanted or last_wanted:   # only the last stage normalises (or limits) and quantises
        clip = model.synthesize(args.synthesize, normalize=False, want_pcm=False, **how)
    if reverb_wanted:
        from gansynth_amd import reverb
        try:   # the room AT the output rate: designed (one channel per channel of the clip, from the one seed) or read
            if args.reverb is not None:
                impulse = reverb.design_impulse(info["sample_rate"], args.reverb, channels=clip.dim(), seed=args.seed, predelay=args.reverb_predelay)
            else:
                impulse = reverb.read_impulse(args.reverb_ir, info["sample_rate"], predelay=args.reverb_predelay)
            clip, pcm, peak = reverb.apply(clip, impulse.to(clip.device), mix=args.reverb_mix, normalize=not last_wanted, want_pcm=not last_wanted)
        except ValueError as e:
            raise SystemExit(str(e))
        info.update(peak=float(peak), reverb_tail=int(impulse.shape[1]) - 1, output_samples=int(clip.shape[-1]))
    if loudness_wanted:   # the clip as the stage before left it; its level comes from the meter, not from that stage's peak
        from gansynth_amd import loudness
        ceiling_db = args.limit if limit_wanted else -1.0
        try:
            limited, pcm, heard = loudness.apply(clip, info["sample_rate"], args.loudness, ceiling_db=ceiling_db,
                                                 lookahead_seconds=args.limit_lookahead, want_pcm=True, **extra)
        except ValueError as e:
            raise SystemExit(str(e))
        info.update(loudness_target=float(args.loudness), loudness_measured=heard["measured_lufs"], loudness_output=heard["output_lufs"],
                    limit_ceiling_db=float(ceiling_db), limit_peak=heard["peak"], limit_min_gain=heard["min_gain"])
    elif limit_wanted:   # the clip as the stage before left it, and that stage's peak
        from gansynth_amd import limiter
        try:
            limited, pcm, out_peak, min_gain = limiter.apply(clip, info["sample_rate"], ceiling_db=args.limit, drive_db=args.limit_drive,
                                                             lookahead_seconds=args.limit_lookahead, peak=info["peak"], want_pcm=True, **extra)
        except ValueError as e:
            raise SystemExit(str(e))
        info.update(limit_ceiling_db=float(args.limit), limit_drive_db=float(args.limit_drive), limit_peak=float(out_peak),
                    limit_min_gain=float(min_gain))
    elif not reverb_wanted:
        _, pcm = model.synthesize(args.synthesize, want_pcm=True, **how)
    if true_peak_wanted:   # what the file reconstructs to: one more detector call, on the limiter's float output
        from gansynth_amd import true_peak
        info.update(true_peak_db=true_peak.measure(limited))
    if restore:
        log(f"restored {model.restored_from}")
    rate = int(model.spectral_params["sample_rate"])
    wavfile.write(args.output, rate=info["sample_rate"], data=pcm.cpu().numpy())
    log(f"{len(info['notes'])} notes kept, {info['dropped']} dropped, {info['total_samples'] / rate:.3f} seconds, "
        f"peak {info['peak']:.4f}: written to {args.output}" + (f" at {info['sample_rate']} Hz" if info["sample_rate"] != rate else "")
        + (f", with a reverb tail of {info['reverb_tail']} samples ({info['reverb_tail'] / info['sample_rate']:.3f} seconds)" if reverb_wanted else "")
        + (f", limited to {args.limit:g} dBFS with {args.limit_drive:g} dB of drive, deepest gain reduction "
           f"{-20.0 * math.log10(max(info['limit_min_gain'], 1e-10)):.2f} dB" if limit_wanted and not loudness_wanted else "")
        + (f", measured {info['loudness_measured']:.2f} LUFS, brought to {info['loudness_output']:.2f} LUFS for a target of {args.loudness:g} "
           f"under a ceiling of {info['limit_ceiling_db']:g} dBFS"
           + (f": the limiter had to work (least gain {info['limit_min_gain']:.4f}) and the output is "
              f"{args.loudness - info['loudness_output']:.2f} LU short of the target" if info["limit_min_gain"] < 1 else "")
           if loudness_wanted else "")
        + (f", true peak {info['true_peak_db']:.2f} dBTP (the ceiling is read in dBTP)" if true_peak_wanted else ""))
    if controllers_wanted:
        counts = info["controls"]
        log(f"controllers: {counts['volume']} volume, {counts['expression']} expression and {counts['pan']} pan events in {info['curve_points']} "
            f"curve points, {info['pedal_extended']} notes held by the pedal")
    if bend_wanted:
        log(f"bend: {sum(info['bends'])} events on {sum(1 for n in info['bends'] if n)} parts in {info['bend_points']} curve points, "
            f"{info['bent_notes']} notes bent")
    if sustain_wanted:
        lags = [m for _, m, _ in info["loops"]]
        log(f"sustain: {info['held_notes']} notes held in {info['sustain_rows']} pieces, loops of {min(lags, default=0)} to {max(lags, default=0)} "
            f"samples, {info['sustain_cut_bent']} held notes cut because they bend")
    return info


def pack_bank(args, pitches, sources, log=print):
    """--pack_bank: host work only (gansynth_amd.bank.pack), before any device is touched."""
    from gansynth_amd import bank
    files = sorted(glob.glob(args.filenames))
    if not files:
        raise SystemExit(f"--pack_bank: --filenames {args.filenames} matches no file")
    header = bank.pack(files, args.pack_bank, pitches=pitches, sources=sources)
    log(f"{header['rows']} of {header['total_records']} notes packed into {args.pack_bank}")
    return header


def main(args):
    check_reverb_args(args)
    check_limit_args(args)
    check_loudness_args(args)
    check_controller_args(args)
    check_true_peak_args(args)
    check_prd_args(args)
    check_kid_args(args)
    if getattr(args, "f0", False) and not args.evaluate:
        raise SystemExit("--f0 applies to --evaluate only")
    if args.pack_bank is not None:
        pack_bank(args, range(24, 85), [0])
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    from gansynth_amd import checkpoint, variables
    from gansynth_amd.bank import NoteBank, bank_input_fn
    from gansynth_amd.dataset import nsynth_input_fn, synthetic_nsynth_input_fn
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict

    torch.manual_seed(rank)   # tf.set_random_seed(0) (:44); one latent stream per rank
    dtype = torch.float32 if args.dtype == "f32" else torch.bfloat16
    device = torch.device("cuda", local_rank)
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    pitches = range(24, 85)
    global_batch = args.batch_size * world

    holder = {}
    pggan = PGGAN(min_resolution=[2, 16], max_resolution=[128, 1024], min_channels=32, max_channels=256,
                  growing_level=lambda: holder["model"].global_step / args.growing_steps)   # :52-55

    def real_input_fn_factory(train):
        if args.synthetic:
            return synthetic_nsynth_input_fn(args.batch_size, pitches, device=device, seed=rank,
                                             num_batches=None if train else args.num_generate_batches)
        if args.bank is not None:   # every rank holds the whole bank and draws its own order from it
            if "bank" not in holder:     # (--train, --evaluate and --generate in one run share one upload)
                holder["bank"] = NoteBank.open(args.bank)
            return bank_input_fn(holder["bank"], args.batch_size, args.num_epochs if train else 1,
                                 shuffle=train, pitches=pitches, sources=[0], device=device, seed=rank)
        files = sorted(glob.glob(args.filenames))
        if world > 1:
            files = files[rank::world] or files
        return nsynth_input_fn(files, args.batch_size, args.num_epochs if train else 1, shuffle=train, pitches=pitches,
                               sources=[0], device=device, seed=rank)

    # (--synthesize alone reads no dataset: its pitches come from the score)
    real_input_fn = real_input_fn_factory(args.train) if (args.train or args.evaluate or args.generate) else None
    model = GANSynth(
        generator=pggan.generator, discriminator=pggan.discriminator,
        real_input_fn=real_input_fn,
        fake_input_fn=lambda: torch.randn(args.batch_size, 256, device=device),   # :70
        spectral_params=Dict(waveform_length=64000, sample_rate=16000, spectrogram_shape=[128, 1024], overlap=0.75),
        hyper_params=Dict(generator_learning_rate=8e-4 * global_batch / 8, generator_beta1=0.0, generator_beta2=0.99,
                          discriminator_learning_rate=8e-4 * global_batch / 8, discriminator_beta1=0.0, discriminator_beta2=0.99,
                          mode_seeking_loss_weight=0.1, real_gradient_penalty_weight=5.0, fake_gradient_penalty_weight=0.0,
                          generator_average_decay=args.generator_ema_decay),
        dtype=dtype, distributed=world > 1, use_graphs=True)
    holder["model"] = model

    if args.train:
        model.train(                                   # gan_synth_main.py:102-109, argument for argument
            model_dir=args.model_dir,                  # (every rank restores, rank 0 saves)
            config=None,                               # (the reference's tf.ConfigProto: nothing of it applies here)
            total_steps=args.total_steps,
            save_checkpoint_steps=args.save_checkpoint_steps,
            save_summary_steps=args.save_summary_steps,
            log_tensor_steps=args.log_tensor_steps,
            log=print if rank == 0 else None)
        if rank == 0:
            print(f"stopped at global_step = {model.global_step}")

    if args.evaluate:   # :111-124, one process
        if world > 1:
            raise SystemExit("--evaluate runs in one process: launch it without torch.distributed")
        if args.synthetic and args.num_generate_batches is None:
            raise SystemExit("--evaluate --synthetic needs --num_generate_batches (synthetic input never ends)")
        no_classifier = args.classifier.lower() == "none"
        if no_classifier and not (args.swd or getattr(args, "f0", False)):
            raise SystemExit("--evaluate --classifier none needs --swd or --f0 (every other figure comes from the pitch classifier)")
        kept = model.real_input_fn   # evaluate runs over an input of its own: --generate after it still has its batches
        model.real_input_fn = real_input_fn_factory(False)
        try:
            print(model.evaluate(
                model_dir=args.model_dir,
                config=None,
                classifier=None if no_classifier else args.classifier,    # the frozen pitch-classifier GraphDef (.pb), or its weights as .safetensors
                input_name="images:0",
                output_names=["features:0", "logits:0"],
                weights=args.weights,
                **(dict(extra_metrics=True, ndb="device") if args.ndb else {}),     # (without the flags the call is the one it was)
                **(dict(swd=True) if args.swd else {}),
                **(dict(f0=True, pitches=pitches) if getattr(args, "f0", False) else {}),
                **(dict(prd=True, prd_k=args.prd_k) if args.prd else {}),
                **(dict(kid=True, kid_subsets=args.kid_subsets, kid_subset_size=args.kid_subset_size) if getattr(args, "kid", False) else {})))
        finally:
            model.real_input_fn = kept

    if args.generate and rank == 0:
        from scipy.io import wavfile
        os.makedirs("samples", exist_ok=True)
        if not args.train:
            real_input_fn = model.real_input_fn
        num_waveforms, batches = 0, 0
        while args.num_generate_batches is None or batches < args.num_generate_batches:
            try:
                # models.py:232-250: labels of the dataset, fresh latents (a resident bank hands over the labels alone)
                labels = real_input_fn.next_labels() if hasattr(real_input_fn, "next_labels") else real_input_fn()[1]
            except StopIteration:
                break
            latents = model.fake_input_fn()
            model._ensure_built(latents.to(dtype), labels.to(dtype))
            if batches == 0 and not args.train:
                from_file = args.weights == "average" and model.g_params.avg is None   # (no decay in this run: the checkpoint's averages)
                path = checkpoint.restore(model, args.model_dir, require_average=from_file)
                if path is None and from_file:
                    raise SystemExit(f"--weights average: {args.model_dir} holds no checkpoint to take the averaged generator from")
                print(f"restored {path}" if path else "no checkpoint found: generating from the initial weights")
            for waveform in model.generate(latents, labels, weights=args.weights, sample_rate=args.output_rate).float().cpu().numpy():
                wavfile.write(f"samples/{num_waveforms}.wav", rate=args.output_rate or 16000, data=waveform)
                num_waveforms += 1
            batches += 1
        print(f"{num_waveforms} waveforms are generated in `samples` directory")

    if args.synthesize is not None:   # one process
        if world > 1:
            raise SystemExit("--synthesize runs in one process: launch it without torch.distributed")
        synthesize_to_wav(model, args, pitches, restore=not args.train)

    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(parser.parse_args())
