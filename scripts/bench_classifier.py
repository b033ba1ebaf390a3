"""Pitch-classifier benchmark (networks.ResNet, GANSynth.evaluate): prints ONE JSON line.

    python scripts/bench_classifier.py [--batch 64] [--iters 10] [--eval-examples 512]
    python scripts/bench_classifier.py --train [--batch 64] [--iters 10] [--out profiles/cls_bench_classifier_train.json]

  forward_images_per_s   {bf16, f32}: classifier forward at --batch, device events around --iters forwards after 3 warm-up ones
  evaluate_examples_per_s  GANSynth.evaluate on synthetic notes (bf16 GAN, fp32 classifier), host clock around the whole call
                           after one warm-up call; the synthetic notes are made on the host by a prefetch thread
  families               {dtype: {family: {ms, launches, flops, bytes, roof_ms, share, bound}}} from gs_prof_records of one forward:
                           the algorithmic flops / bytes of each launch from its shapes, roof = max(flops / peak, bytes / HBM) per launch,
                           share = roof / measured time; peak: the dtype's dense MFMA rate for the 3x3 convs, the fp32 vector rate for the
                           VALU kernels (stem, projections).  Random weights: the timings do not depend on their values.
  --train                the training leg instead (fp32, full size): train_step_ms = ResNet.forward_backward + momentum_step, device events
                           around --iters steps after 3 warm-up ones, next to forward_ms["f32"] of the same run; families of one step as
                           above (the backward's launches included); hbm_fraction = bytes / (8 TB/s x measured time) of the two
                           HBM-bound families of the backward (gn_bwd, momentum)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_TF = {"bf16": 2500.0, "f32": 157.3}   # MI355X dense MFMA peaks (TFLOP/s)
VALU_TF = 157.3                            # fp32 vector peak
HBM_GBPS = 8000.0
FAMILY = {0: "conv3x3", 1: "conv3x3", 40: "stem_pool", 41: "projection", 42: "gn_stats", 43: "gn_apply", 44: "head", 45: "weight_std",
          46: "max_pool", 50: "gn_bwd", 51: "head_bwd", 52: "weight_std_batch", 53: "weight_std_bwd", 54: "max_pool_bwd", 55: "stem_wgrad",
          56: "projection_bwd_data", 57: "projection_bwd_weight", 58: "softmax_xent", 59: "momentum"}


def _net():
    from gansynth_amd.networks import ResNet
    net = ResNet.pitch_classifier()
    rng = np.random.default_rng(0)
    state = {}
    for k, v in net.create_variables().items():
        shape = tuple(v.shape)
        if k.endswith("/gamma"):
            state[k] = 1.0 + 0.1 * rng.standard_normal(shape)
        elif k.endswith("/beta") or k.endswith("/bias"):
            state[k] = 0.1 * rng.standard_normal(shape)
        else:
            state[k] = rng.standard_normal(shape) * np.sqrt(2.0 / max(1, int(np.prod(shape[:-1]))))
    net.load_state_dict({k: np.asarray(v, np.float32) for k, v in state.items()})
    return net


def _forward_rate(net, dtype, batch, iters):
    x = torch.randn(batch, 2, 128, 1024, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
    for _ in range(3):
        net(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        net(x)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    return batch / (ms * 1e-3), ms


def _train_step(net, x, y):
    out = net.forward_backward(x, y)
    net.momentum_step(0.032, 0.9, True, 1e-4)
    return out


def _train_rate(net, batch, iters):
    x = torch.randn(batch, 2, 128, 1024, device="cuda").contiguous(memory_format=torch.channels_last)
    y = torch.eye(61, device="cuda")[torch.randint(0, 61, (batch,), device="cuda")]
    for _ in range(3):
        _train_step(net, x, y)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        _train_step(net, x, y)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _families(net, dtype, batch, train=False):
    from gansynth_amd import kernels
    K = kernels.get()
    x = torch.randn(batch, 2, 128, 1024, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
    y = torch.eye(61, device="cuda")[torch.randint(0, 61, (batch,), device="cuda")]
    run = (lambda: _train_step(net, x, y)) if train else (lambda: net(x))
    run()
    torch.cuda.synchronize()
    K.prof_enable(1)
    run()
    torch.cuda.synchronize()
    recs = K.prof_records()
    K.prof_collect()
    K.prof_enable(0)
    name = "bf16" if dtype == torch.bfloat16 else "f32"
    out = {}
    for ms, fl, by, desc in recs:
        fam = FAMILY.get(desc[0], "conv3x3" if desc[0] < 10 else "conv3x3_wgrad" if desc[0] < 20 else f"kind{desc[0]}")   # (2, 3: the stride-2 data gradients)
        peak = MFMA_TF[name] if fam.startswith("conv3x3") else VALU_TF
        tf, tb = fl / (peak * 1e12) * 1e3, by / (HBM_GBPS * 1e9) * 1e3
        d = out.setdefault(fam, dict(ms=0.0, launches=0, flops=0.0, bytes=0.0, roof_ms=0.0, flop_roof_ms=0.0, byte_roof_ms=0.0))
        d["ms"] += ms
        d["launches"] += 1
        d["flops"] += fl
        d["bytes"] += by
        d["roof_ms"] += max(tf, tb)
        d["flop_roof_ms"] += tf
        d["byte_roof_ms"] += tb
    for d in out.values():
        d["share"] = d["roof_ms"] / d["ms"] if d["ms"] > 0 else None
        d["hbm_fraction"] = d["byte_roof_ms"] / d["ms"] if d["ms"] > 0 else None
        d["bound"] = "compute" if d.pop("flop_roof_ms") >= d.pop("byte_roof_ms") else "hbm"
    # the 512-channel 4 x 32 convs of stage 4 on their own (desc = kind, N, Hb, Wb, IC, OC, ...)
    st4 = [(ms, fl) for ms, fl, by, desc in recs if desc[0] in (0, 1) and desc[5] == 512]
    if st4 and not train:
        t, f = sum(r[0] for r in st4), sum(r[1] for r in st4)
        out["conv3x3"]["stage4_share"] = f / (MFMA_TF[name] * 1e12) * 1e3 / t
    return out


def _evaluate_rate(examples, gan_batch):
    from gansynth_amd import variables
    from gansynth_amd.dataset import synthetic_nsynth_input_fn
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict
    net = _net()
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    pg = PGGAN(min_resolution=[2, 16], max_resolution=[128, 1024], min_channels=32, max_channels=256, growing_level=1.0)
    spectral = Dict(waveform_length=64000, sample_rate=16000, spectrogram_shape=[128, 1024], overlap=0.75)
    hyper = Dict(generator_learning_rate=8e-4, generator_beta1=0.0, generator_beta2=0.99, discriminator_learning_rate=8e-4,
                 discriminator_beta1=0.0, discriminator_beta2=0.99, mode_seeking_loss_weight=0.1, real_gradient_penalty_weight=5.0,
                 fake_gradient_penalty_weight=0.0)

    def run(n):
        real = synthetic_nsynth_input_fn(gan_batch, range(24, 85), num_batches=n // gan_batch, device=torch.device("cuda"), seed=0, prefetch=4)
        model = GANSynth(pg.generator, pg.discriminator, real, lambda: torch.randn(gan_batch, 256, device="cuda"), spectral, hyper,
                         dtype=torch.bfloat16)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fid = model.evaluate(None, None, net, "images:0", ["features:0", "logits:0"])["frechet_inception_distance"]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, fid

    run(gan_batch * 2)
    dt, fid = run(examples)
    return examples / dt, dt, fid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--eval-examples", type=int, default=576)
    ap.add_argument("--gan-batch", type=int, default=32)
    ap.add_argument("--no-evaluate", action="store_true")
    ap.add_argument("--train", action="store_true", help="the training leg: fp32 step time and per-family table")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_classifier.py needs a GPU"
    net = _net()
    if args.train:
        rate, fwd_ms = _forward_rate(net, torch.float32, args.batch, args.iters)
        step_ms = _train_rate(net, args.batch, args.iters)
        res = dict(metric="pitch_classifier_train", batch=args.batch, dtype="f32", forward_ms=dict(f32=fwd_ms), forward_images_per_s=dict(f32=rate),
                   train_step_ms=step_ms, train_images_per_s=args.batch / (step_ms * 1e-3), step_over_forward=step_ms / fwd_ms,
                   families=_families(net, torch.float32, args.batch, train=True))
        res["family_ms_total"] = sum(d["ms"] for d in res["families"].values())
        line = json.dumps(res)
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
        print(line)
        return
    res = dict(metric="pitch_classifier", batch=args.batch, forward_images_per_s={}, forward_ms={}, families={})
    for name, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        rate, ms = _forward_rate(net, dt, args.batch, args.iters)
        res["forward_images_per_s"][name], res["forward_ms"][name] = rate, ms
        res["families"][name] = _families(net, dt, args.batch)
    if not args.no_evaluate:
        rate, secs, fid = _evaluate_rate(args.eval_examples, args.gan_batch)
        res["evaluate_examples_per_s"] = rate
        res["evaluate"] = dict(examples=args.eval_examples, seconds=secs, fid=fid, gan_batch=args.gan_batch)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
