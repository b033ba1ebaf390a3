"""GPU: the PGGAN G+D path end to end on the HIP kernels vs the oracle (fp32, 1e-3 relative) --
forward, both losses (R1 + mode-seeking double-backward), every parameter gradient and one
TF-Adam update; config[0] of BASELINE.json (2x16 stage, batch 4 -- SURVEY.md D1/D2) against the
committed golden fixture; fade-in regimes; the fully grown full-size iteration (configs[1]) in fp32 (batch 4)
and in bf16 (batch 8) with leaky-relu sign flips counted and bounded instead of tolerated."""
import os

import numpy as np
import pytest
import torch

from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def relerr(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float()
    return float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)


def make(level, store, full=True, dtype=torch.float32, hyper=None):
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.models import GANSynth
    from gansynth_amd.utils import Dict
    kw = dict(min_resolution=[2, 16], max_resolution=[128, 1024], min_channels=32, max_channels=256) if full else \
        dict(min_resolution=[2, 16], max_resolution=[16, 128], min_channels=32, max_channels=64)
    pg, opg = PGGAN(growing_level=level, **kw), R.PGGAN(growing_level=level, **kw)
    model = GANSynth(pg.generator, pg.discriminator, None, None, None, Dict(hyper or R.DEFAULT_HYPER), dtype=dtype,
                     keep_gradients=True)   # (the parity tests read p.grad after the optimizer step)
    return pg, opg, model


def replaying_graphs(model, key=None):
    """The trainer replays captured runs in the growing regime `key` = (head depth, not fading): one graph per run, or the merged pair of
    train_step() on one GPU (models.GANSynth._train_step_merged)."""
    if model._merged is not None:
        return key is None or tuple(model._merged["key"][:2]) == tuple(key)
    return set(model._graphs) == {"d", "g"} and (key is None or model._graph_key == tuple(key))


def cuda(t):
    return t.cuda().contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.cuda()


def flip_report(masks, recorded, what, max_fraction=2e-5, near=1e-4):
    """Leaky-relu sign disagreements between the HIP pass (`masks`, from functional.activation_tap) and the oracle's nominal pass
    (`recorded`, from lrelu_tape("record")), matched call by call by (network name, occurrence).  Every disagreement must sit at a
    pre-activation the oracle itself holds within `near` x the tensor's rms of zero (i.e. inside fp32 round-off of the kink), and
    there must be few of them.  Returns (flips, elements, largest |x| / rms among the flipped)."""
    def keyed(calls):
        seen, out = {}, {}
        for name, items in calls:
            out[(name, seen.get(name, 0))] = items
            seen[name] = seen.get(name, 0) + 1
        return out
    hip, ora = keyed(masks), keyed(recorded)
    assert set(hip) == set(ora), (sorted(hip), sorted(ora))
    flips = total = 0
    worst_ratio = 0.0
    for key in hip:
        assert len(hip[key]) == len(ora[key]), (key, len(hip[key]), len(ora[key]))
        for i, (m, x) in enumerate(zip(hip[key], ora[key])):
            assert m.shape == x.shape, (key, i, tuple(m.shape), tuple(x.shape))
            wrong = m != (x > 0)
            n = int(wrong.sum())
            total += m.numel()
            if n:
                flips += n
                rms = float(x.double().pow(2).mean().sqrt())
                worst = float(x[wrong].abs().max())
                worst_ratio = max(worst_ratio, worst / rms)
                assert worst <= near * rms, f"{what}: {key} leaky_relu #{i}: sign differs at |x| = {worst:.3e} (rms {rms:.3e})"
    assert flips <= max(2, max_fraction * total), f"{what}: {flips} sign flips in {total} pre-activations"
    return flips, total, worst_ratio


def aligned(masks, oracle_order):
    """Reorder the HIP tap's calls into the oracle's call order (name, occurrence)."""
    seen, by_key = {}, {}
    for name, items in masks:
        by_key[(name, seen.get(name, 0))] = items
        seen[name] = seen.get(name, 0) + 1
    seen, out = {}, []
    for name in oracle_order:
        out.append((name, by_key[(name, seen.get(name, 0))]))
        seen[name] = seen.get(name, 0) + 1
    return out


def rel_l2(a, b):
    a, b = a.detach().double().flatten().cpu(), b.detach().double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def check_adam_update(params, before, hip_grads, oracle_before, oracle_after, oracle_grads, hyper, which, strict_vs_oracle=True):
    """The optimizer step as an UPDATE (p_after - p_before), not as parameters: weights are O(1) and the first TF-Adam step moves
    every element by lr = 8e-4 (m = (1 - beta1) g, sqrt(v) = sqrt(1 - beta2) |g|, lr_t = lr sqrt(1 - beta2) / (1 - beta1): the step is
    lr * sign(g) wherever sqrt(v) >> eps), so a comparison of the parameters themselves at 2e-3 of max|p| ~ 2 could not even see a
    sign-flipped update.  (i) Against oracle.adam_tf_step applied to the HIP path's OWN gradients from the same starting point:
    every element, 1e-3 of lr (about three fp32 ulps of a weight) -- the kernel's arithmetic inside the step (eps outside the bias
    correction, the 1/world scale, m and v from zero).  (ii) Against the oracle's own update (its gradients): every element whose
    oracle gradient is at least 1 % of its tensor's largest (there the sign cannot change within the gradient tolerance) and large
    against eps, at 1e-2 of lr."""
    lr, b1, b2 = hyper[which + "_learning_rate"], hyper[which + "_beta1"], hyper[which + "_beta2"]
    lr_t = lr   # (the size of a first step, see above)
    own = {k: v.cpu().clone() for k, v in before.items()}
    grads = {k: hip_grads[k].cpu() for k in own}
    R.adam_tf_step(own, grads, {k: torch.zeros_like(v) for k, v in own.items()}, {k: torch.zeros_like(v) for k, v in own.items()}, 1, lr, b1, b2)
    worst_own = worst_ref = 0.0
    for k, p in params.named.items():
        upd = p.data.cpu() - before[k].cpu()
        assert float(upd.abs().max()) <= 1.01 * lr_t + 2.5e-7 * float(before[k].abs().max()), (k, float(upd.abs().max()), lr_t)
        d_own = float((upd - (own[k] - before[k].cpu())).abs().max())
        worst_own = max(worst_own, d_own / lr_t)
        assert d_own <= 1e-3 * lr_t + 2.5e-7 * float(before[k].abs().max()), f"{k}: update differs from TF-Adam on the same gradient by {d_own / lr_t:.3e} lr"
        g = oracle_grads[k]
        big = g.abs() >= max(1e-2 * float(g.abs().max()), 1e-5)   # (sqrt(v) = 0.1 |g| is then >= 100 eps: the element moves by ~lr)
        if strict_vs_oracle and bool(big.any()):
            ref = (oracle_after[k].detach() - oracle_before[k].detach())[big]
            d_ref = float((upd[big] - ref).abs().max())
            worst_ref = max(worst_ref, d_ref / lr_t)
            assert d_ref <= 1e-2 * lr_t + 2.5e-7 * float(before[k].abs().max()), f"{k}: update differs from the oracle's by {d_ref / lr_t:.3e} lr"
            assert float(ref.abs().min()) > 0.9 * lr_t   # (these elements did move by ~lr_t: the check above is not vacuous)
    return worst_own, worst_ref


def run_step_parity(pg, opg, model, store, batch, res, tol=1e-3, grad_tol=None, verbose=False, dtype=torch.float32,
                    flip_fraction=2e-5, flip_near=1e-4, metric=None, hyper=None):
    """One full iteration (D update then G update, each on its own batch) on the HIP path against the oracle: forward, both
    losses, EVERY parameter gradient (first-order + the R1 / mode-seeking double-backward terms) and the TF-Adam update.

    leaky_relu is the one ill-conditioned op of the graph (piecewise linear: a pre-activation within fp32 round-off of 0 can land on
    either side, and the unit's gradient then differs 5x).  So each run is compared twice: (i) the sign pattern of every
    leaky_relu of the HIP pass against the oracle's nominal pass -- disagreements are counted and each must sit inside round-off
    of the kink (flip_report); (ii) every gradient against the oracle evaluated on the HIP pass's linear pieces
    (lrelu_tape("override")), at `grad_tol` for every tensor without exception."""
    from gansynth_amd import functional as F
    grad_tol = grad_tol or tol / 5
    relerr = metric or globals()["relerr"]
    lat, lab, real = R.synthetic_batch(batch, rank=0, image_shape=(2, *res))
    lat2, lab2, _ = R.synthetic_batch(batch, rank=1, image_shape=(2, *res))
    if dtype != torch.float32:   # both sides see the inputs as the storage dtype holds them
        lat, real, lat2 = (t.to(dtype).float() for t in (lat, real, lat2))
    base_cuda = globals()["cuda"]
    cuda = lambda t: base_cuda(t).to(dtype)
    gp, dp = opg.init_params(seed=0, bias_std=0.1)
    model._build(cuda(lat), cuda(lab))
    store.load_state_dict({**gp, **dp})
    tr = R.Trainer(opg, gp, dp, hyper or R.DEFAULT_HYPER)
    # forward
    with torch.no_grad():
        fake = pg.generator(cuda(lat), cuda(lab))
        feats, logits = pg.discriminator(cuda(real), cuda(lab))
        ofake = opg.generator(gp, lat, lab)
        ofeats, ologits = opg.discriminator(dp, real, lab)
    assert relerr(fake, ofake) < tol, f"generator images {relerr(fake, ofake):.2e}"
    assert relerr(feats, ofeats) < tol and relerr(logits, ologits) < tol
    stats = {}
    # ---- D run: G(z) (no grad), D(real) + R1 double-backward, D(fake); everything on the HIP path
    d_before = {k: p.data.clone() for k, p in model.d_params.named.items()}
    od_before = {k: t.detach().clone() for k, t in tr.d.items()}
    with F.activation_tap() as tap:
        d_loss = model.discriminator_step(cuda(lat), cuda(lab), cuda(real))
    d_grads = {k: p.grad.clone() for k, p in model.d_params.named.items()}
    masks = tap.masks()
    with R.lrelu_tape("record") as rec:
        nominal_loss = R.discriminator_loss(opg, tr.g, tr.d, lat, lab, real, tr.hyper)
    stats["d_flips"] = flip_report(masks, rec.calls, "D run", flip_fraction, flip_near)
    assert abs(float(d_loss) - float(nominal_loss.detach())) <= tol * max(1.0, abs(float(nominal_loss.detach()))), (float(d_loss), float(nominal_loss.detach()))
    with R.lrelu_tape("override", aligned(masks, [n for n, _ in rec.calls])):
        od_loss, od_grads = tr.d_step(lat, lab, real)
    del rec
    assert abs(float(d_loss) - float(od_loss)) <= tol * max(1.0, abs(float(od_loss))), (float(d_loss), float(od_loss))
    bad = {k: relerr(d_grads[k], od_grads[k]) for k in od_grads if float(od_grads[k].abs().max()) > 0}
    stats["d_grad_worst"] = max(bad.values())
    assert max(bad.values()) < grad_tol, sorted(bad.items(), key=lambda kv: -kv[1])[:5]
    zero = [k for k in od_grads if float(od_grads[k].abs().max()) == 0]
    assert all(float(d_grads[k].abs().max()) == 0 for k in zero)  # untaken branches: exactly zero gradient
    stats["d_update"] = check_adam_update(model.d_params, d_before, d_grads, od_before, tr.d, od_grads, tr.hyper, "discriminator",
                                          strict_vs_oracle=dtype == torch.float32)
    with torch.no_grad():   # the G run starts from identical discriminators (Adam's first step is sign-like: lr * g / |g|)
        for k, p in model.d_params.named.items():
            tr.d[k].copy_(p.data.cpu())
    # ---- G run: G(z) + mode-seeking double-backward, D(G(z)); everything on the HIP path
    g_before = {k: p.data.clone() for k, p in model.g_params.named.items()}
    og_before = {k: t.detach().clone() for k, t in tr.g.items()}
    with F.activation_tap() as tap:
        g_loss = model.generator_step(cuda(lat2), cuda(lab2))
    g_grads = {k: p.grad.clone() for k, p in model.g_params.named.items()}
    masks = tap.masks()
    with R.lrelu_tape("record") as rec:
        nominal_loss = R.generator_loss(opg, tr.g, tr.d, lat2, lab2, tr.hyper)
    stats["g_flips"] = flip_report(masks, rec.calls, "G run", flip_fraction, flip_near)
    assert abs(float(g_loss) - float(nominal_loss.detach())) <= tol * max(1.0, abs(float(nominal_loss.detach()))), (float(g_loss), float(nominal_loss.detach()))
    with R.lrelu_tape("override", aligned(masks, [n for n, _ in rec.calls])):
        og_loss, og_grads = tr.g_step(lat2, lab2)
    del rec
    assert abs(float(g_loss) - float(og_loss)) <= tol * max(1.0, abs(float(og_loss))), (float(g_loss), float(og_loss))
    bad = {k: relerr(g_grads[k], og_grads[k]) for k in og_grads if float(og_grads[k].abs().max()) > 0}
    stats["g_grad_worst"] = max(bad.values())
    assert max(bad.values()) < grad_tol, sorted(bad.items(), key=lambda kv: -kv[1])[:5]
    zero = [k for k in og_grads if float(og_grads[k].abs().max()) == 0]
    assert all(float(g_grads[k].abs().max()) == 0 for k in zero)
    stats["g_update"] = check_adam_update(model.g_params, g_before, g_grads, og_before, tr.g, og_grads, tr.hyper, "generator",
                                          strict_vs_oracle=dtype == torch.float32)
    assert model.global_step == 1
    if verbose:
        print("step parity:", stats)
    return fake, feats, logits, d_loss, g_loss, d_grads, g_grads


def test_config0_2x16_stage_batch4_vs_oracle_and_golden(gpu_store):
    pg, opg, model = make(0.0, gpu_store)
    fake, feats, logits, d_loss, g_loss, d_grads, g_grads = run_step_parity(pg, opg, model, gpu_store, 4, (128, 1024))
    gold = np.load(os.path.join(GOLD, "pggan_2x16_b4.npz"))
    up = fake.float().cpu()
    assert torch.equal(up[:, :, ::64, ::64].repeat_interleave(64, 2).repeat_interleave(64, 3), up)  # nearest upscale: bit-exact blocks
    assert relerr(up[:, :, ::64, ::64], torch.from_numpy(gold["fake_2x16"])) < 1e-3
    assert relerr(feats, torch.from_numpy(gold["features"])) < 1e-3
    assert relerr(logits, torch.from_numpy(gold["logits"])) < 1e-3
    assert abs(float(d_loss) - float(gold["d_loss"])) < 1e-3 * max(1.0, abs(float(gold["d_loss"])))
    assert abs(float(g_loss) - float(gold["g_loss"])) < 1e-3 * max(1.0, abs(float(gold["g_loss"])))
    for k, g in list(d_grads.items()) + list(g_grads.items()):
        ref = float(gold["gradnorm/" + k])
        assert abs(float(g.double().norm()) - ref) <= 2e-2 * ref + 1e-12, k


@pytest.mark.parametrize("level", [0.12, 0.25, 0.6, 1.0])
def test_fade_regimes_reduced_pggan(gpu_store, level):
    """2x16 .. 16x128 PGGAN (depth 3): level 0.12 -> depth 1 fade, 0.25 -> 2, 0.6 -> 3, 1.0 fully grown."""
    pg, opg, model = make(level, gpu_store, full=False)
    run_step_parity(pg, opg, model, gpu_store, 4, (16, 128))


@pytest.mark.parametrize("level", [0.25, 1.0])
def test_penalty_on_the_generator_distribution_vs_oracle(gpu_store, level):
    """`fake_gradient_penalty_weight` (/root/reference models.py:50-54; 0 in gan_synth_main.py:87): the zero-centred penalty on
    tf.gradients(fake_logits, [fake_images]), i.e. the R1 double-backward kernels on the FAKE batch, through the HIP path -- loss,
    every discriminator gradient and the update against oracle.torch_ref at weight 1 (the per-sample loss algebra runs: the one-launch
    loss kernel carries one penalty term).  The term is really there: the oracle's loss moves when it is switched off."""
    hyper = dict(R.DEFAULT_HYPER, fake_gradient_penalty_weight=1.0)
    pg, opg, model = make(level, gpu_store, full=False, hyper=hyper)
    _, _, _, d_loss, _, _, _ = run_step_parity(pg, opg, model, gpu_store, 4, (16, 128), hyper=hyper)
    lat, lab, real = R.synthetic_batch(4, rank=0, image_shape=(2, 16, 128))
    gp, dp = opg.init_params(seed=0, bias_std=0.1)
    off = float(R.discriminator_loss(opg, gp, dp, lat, lab, real, dict(hyper, fake_gradient_penalty_weight=0.0)).detach())
    on = float(R.discriminator_loss(opg, gp, dp, lat, lab, real, hyper).detach())
    assert on > off + 1e-4 * abs(off), (on, off)
    assert abs(float(d_loss) - on) <= 1e-3 * max(1.0, abs(on))


def test_channel_counts_that_are_not_powers_of_two_are_refused_loudly(gpu_store):
    """The pixel-norm kernels (forward and every gradient form) take channel counts that are powers of two in 4..1024 -- every
    count the reference configuration produces (min_channels << k, gan_synth_main.py:51-54).  A PGGAN configured with 48 / 96 channels
    is refused with the library's own message at its first norm, never routed somewhere silently; the capability query the
    autograd layer uses for the bias-summing backward says the same."""
    from gansynth_amd import _lib, kernels
    from gansynth_amd.networks import PGGAN
    K = kernels.get()
    assert K.norm_bwd_bias_ok(64) and K.norm_bwd_bias_ok(256, torch.bfloat16) and not K.norm_bwd_bias_ok(48) and not K.norm_bwd_bias_ok(96)
    pg = PGGAN(growing_level=1.0, min_resolution=[2, 16], max_resolution=[8, 64], min_channels=48, max_channels=96)
    lat, lab, _ = R.synthetic_batch(4, rank=0, image_shape=(2, 8, 64))
    with pytest.raises(_lib.GansynthHipError, match="power of two"):
        pg.generator(cuda(lat), cuda(lab))


def test_fully_grown_full_size_forward(gpu_store):
    """BASELINE.json configs[1] shape (128x1024x2, fully grown), forward of both networks, batch 4."""
    pg, opg, model = make(1.0, gpu_store)
    lat, lab, real = R.synthetic_batch(4, rank=0)
    gp, dp = opg.init_params(seed=0, bias_std=0.1)
    model._build(cuda(lat), cuda(lab))
    gpu_store.load_state_dict({**gp, **dp})
    with torch.no_grad():
        fake = pg.generator(cuda(lat), cuda(lab))
        feats, logits = pg.discriminator(cuda(real), cuda(lab))
        ofake = opg.generator(gp, lat, lab)
        ofeats, ologits = opg.discriminator(dp, real, lab)
    assert fake.shape == (4, 2, 128, 1024)
    assert relerr(fake, ofake) < 1e-3
    assert relerr(feats, ofeats) < 1e-3 and relerr(logits, ologits) < 1e-3
    # ... and against the committed full-size fixture (SURVEY.md 8c pin 2: float64 checksums + 64 sampled elements of the outputs and
    # of every leaky_relu output of this very forward, generated by tests/golden/make_golden.py): the HIP path is pinned to a file,
    # not only to an oracle run of the same session
    from gansynth_amd import functional as F
    from tests.golden import make_golden as MG
    gold = np.load(os.path.join(GOLD, "pggan_full_b4.npz"))
    with torch.no_grad(), F.activation_tap() as tap:
        fake = pg.generator(cuda(lat), cuda(lab))
        feats, logits = pg.discriminator(cuda(real), cuda(lab))
    tensors = {"generator/images": fake, "discriminator/features": feats, "discriminator/logits": logits}
    for name, zs in tap.calls:
        for i, z in enumerate(zs):
            tensors["%s/leaky_relu_%02d" % (name, i)] = z
    keys = sorted(k[len("sum/"):] for k in gold.files if k.startswith("sum/"))
    assert keys == sorted(tensors), (keys, sorted(tensors))
    for key in keys:
        a = tensors[key].detach().double().cpu().contiguous().flatten().numpy()   # logical NCHW order, like the oracle's
        assert a.size == int(gold["numel/" + key]), key
        sumabs = float(gold["sumabs/" + key])
        assert abs(np.abs(a).sum() - sumabs) <= 1e-4 * sumabs, (key, np.abs(a).sum(), sumabs)
        assert abs(a.sum() - float(gold["sum/" + key])) <= 1e-4 * sumabs, (key, a.sum(), float(gold["sum/" + key]))
        want = gold["samples/" + key].astype(np.float64)
        got = a[MG.sample_indices(a.size, key)]
        rms = float(np.sqrt(np.mean(np.square(a))))
        assert np.abs(got - want).max() <= 1e-3 * max(rms, np.abs(want).max()), (key, np.abs(got - want).max(), rms)


def test_fully_grown_full_size_step_vs_oracle(gpu_store):
    """BASELINE.json configs[1] shape in fp32: the FULL iteration at 128x1024x2, fully grown, batch 4 -- forward, both losses, every
    parameter gradient including the R1 / mode-seeking double-backward terms, TF-Adam -- against the oracle.  At this size the conv
    kernels run their production tile configurations (resident weights, 256-pixel tiles, two blocks per CU, 64x64 weight-gradient
    tiles, multi-source deferred weight gradients), which the small-shape tests do not reach."""
    pg, opg, model = make(1.0, gpu_store)
    run_step_parity(pg, opg, model, gpu_store, 4, (128, 1024), verbose=True)


def test_full_size_bf16_step_vs_oracle_on_its_linear_pieces(gpu_store):
    """BASELINE.json configs[1] exactly as benchmarked -- batch 8, bf16 storage / fp32 accumulation, fully grown 128x1024x2 -- one
    full iteration against the oracle.  bf16 rounds every stored activation to 8 mantissa bits, so ~0.1 % of the leaky_relu units
    per layer land on the other side of the kink than in fp32 and the raw gradients of this random-init 14-layer chain differ by
    15-30 % in relative L2 from an fp32 evaluation (scripts/bf16_vs_f32.py) -- a property of the dtype, not of the kernels.  What
    the kernels owe is the right arithmetic on the pieces they chose: the oracle is evaluated on the bf16 pass's own leaky_relu
    masks and every gradient tensor must agree in relative L2 (no cosine, no tensor exempted).  The sign disagreements themselves
    are bounded too: each within bf16 round-off (2^-8 of the tensor's rms) of zero."""
    pg, opg, model = make(1.0, gpu_store, dtype=torch.bfloat16)
    # measured (MI355X, round 2): worst gradient tensor 1.8e-2 (D run) / 2.1e-2 (G run) relative L2; 0.19 % / 0.24 % of the
    # pre-activations change side, the farthest one 8.5 % of its tensor's rms from zero (14 layers of accumulated bf16 rounding)
    run_step_parity(pg, opg, model, gpu_store, 8, (128, 1024), tol=3e-2, grad_tol=3e-2, verbose=True, dtype=torch.bfloat16,
                    flip_fraction=5e-3, flip_near=0.15, metric=rel_l2)


def test_bf16_path_tracks_fp32(gpu_store):
    """bf16 storage / fp32 accumulate (BASELINE.json configs[1] dtype): the same step as fp32 within bf16 rounding.
    Forward outputs within 2 % rms (10 % max) of the tensor scale, both losses within 3 %, gradient direction (cosine) > 0.95
    for the large tensors."""
    from gansynth_amd import variables
    lat, lab, real = R.synthetic_batch(4, rank=0, image_shape=(2, 16, 128))
    res = {}
    for dtype in (torch.float32, torch.bfloat16):
        variables.set_default_store(variables.VariableStore(device="cuda"))
        pg, opg, model = make(1.0, variables.default_store(), full=False, dtype=dtype)
        gp, dp = opg.init_params(seed=0, bias_std=0.1)
        model._build(cuda(lat), cuda(lab))
        variables.default_store().load_state_dict({**gp, **dp})
        c = lambda t: cuda(t).to(dtype)
        with torch.no_grad():
            fake = pg.generator(c(lat), c(lab))
            _, logits = pg.discriminator(c(real), c(lab))
        d_loss = model.discriminator_step(c(lat), c(lab), c(real))
        d_grads = {k: p.grad.clone() for k, p in model.d_params.named.items()}
        g_loss = model.generator_step(c(lat), c(lab))
        g_grads = {k: p.grad.clone() for k, p in model.g_params.named.items()}
        res[dtype] = (fake.float(), logits.float(), float(d_loss), float(g_loss), d_grads, g_grads)
    f32, b16 = res[torch.float32], res[torch.bfloat16]
    def rms(a, b):
        return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
    assert rms(b16[0].cpu(), f32[0].cpu()) < 2e-2 and relerr(b16[0].cpu(), f32[0].cpu()) < 1e-1
    assert rms(b16[1].cpu(), f32[1].cpu()) < 3e-2
    assert abs(b16[2] - f32[2]) < 3e-2 * max(1.0, abs(f32[2])) and abs(b16[3] - f32[3]) < 3e-2 * max(1.0, abs(f32[3]))
    for grads_b, grads_f in ((b16[4], f32[4]), (b16[5], f32[5])):
        for k in grads_f:
            a, b = grads_b[k].flatten().double(), grads_f[k].flatten().double()
            if b.numel() >= 4096 and float(b.norm()) > 0:
                cos = float((a @ b) / (a.norm() * b.norm() + 1e-30))
                assert cos > 0.95, (k, cos)



def _same_up_to_accumulation_order(a, b, what, far_fraction=2e-2):
    """Two schedules of the same iteration agree up to the association of fp32 gradient sums: autograd runs independent
    branches in an order given by THREAD-LOCAL node-creation counters (the second-order graphs are created on the engine's
    device thread), so a tensor with three or more gradient contributions -- a multi-consumer activation, the dense weights
    fed by the real pass, the fake pass and the R1 term -- may be summed as (a+b)+c in one run and (a+c)+b in another.  A
    captured graph freezes one such order.  Everything else is deterministic -- in particular the folds of the deferred weight gradients
    associate an entry's sum by the ENTRY's own shape, never by what else shares the launch (a bucketed flush batches them differently) --
    hence a few-ulp tolerance rather than equality."""
    if isinstance(a, float):
        # (a loss of a LATER iteration sees those steps through the forward pass: 2e-4 ... 2e-3 seen between schedules that associate one sum
        #  differently, bit-identical when they do not)
        assert abs(a - b) <= 3e-3 * max(1.0, abs(a)), (what, a, b)
    else:
        # Parameters after a few TF-Adam steps: with beta1 = 0 the first steps are lr * g / (sqrt(1 - beta2) |g| + eps) ~ lr * sign(g) whatever the
        # gradient's size, so an element whose gradient is itself of the size of the sum's round-off (a reassociated fp32 sum moves it by ~1e-7 of
        # the tensor's scale) may step the OTHER way in one schedule: 2 lr = 1.6e-3 apart after one step, and the forward pass then carries the
        # difference on, so that more elements follow in the next step (0.2-0.3 % of the discriminator's after three iterations, seen).  Everything
        # else must agree to 1e-5, at most two elements in a hundred may be further apart, and none by more than a few steps' worth.  The sharp
        # statement -- same arithmetic, another order -- is made where nothing amplifies it: test_replayed_iterations_reproduce_the_eager_gradients
        # compares every replayed schedule with the eager one with both learning rates at zero, and schedules that issue the same launches in
        # the same order are held to bit-identity (forked vs plain graphs, one graph vs the pair).
        diff, scale = (a - b).abs(), float(a.abs().max())
        far = diff > 1e-5 * scale
        assert float(far.float().mean()) <= far_fraction, (what, float(far.float().mean()), float(diff.max()), scale)
        assert float(diff.max()) <= 1e-2 * max(scale, 1.0), (what, float(diff.max()), scale)


def test_hipgraph_replay_equals_eager(gpu_store):
    """Fully grown regime: replaying the captured forward+backward gives the same losses / parameters as eager launches
    (up to the order of fp32 gradient accumulation, see _same_up_to_accumulation_order)."""
    from gansynth_amd import variables
    out = {}
    for graphs in (False, True):
        variables.set_default_store(variables.VariableStore(device="cuda"))
        pg, opg, model = make(1.0, variables.default_store(), full=False)
        model.use_graphs = graphs
        gp, dp = opg.init_params(seed=0, bias_std=0.1)
        losses = []
        for step in range(3):
            lat, lab, real = R.synthetic_batch(4, rank=step, image_shape=(2, 16, 128))
            if step == 0:
                model._build(cuda(lat), cuda(lab))
                variables.default_store().load_state_dict({**gp, **dp})
            losses.append(float(model.discriminator_step(cuda(lat), cuda(lab), cuda(real))))
            losses.append(float(model.generator_step(cuda(lat), cuda(lab))))
        out[graphs] = (losses, model.d_params.flat.clone(), model.g_params.flat.clone())
        if graphs:
            assert set(model._graphs) == {"d", "g"}
    for i, (a, b) in enumerate(zip(out[False][0], out[True][0])):
        _same_up_to_accumulation_order(a, b, f"loss {i}")
    _same_up_to_accumulation_order(out[False][1], out[True][1], "discriminator parameters")
    _same_up_to_accumulation_order(out[False][2], out[True][2], "generator parameters")


@pytest.mark.parametrize("graphs", [False, True])
def test_optimizer_step_clears_the_gradient_it_consumed(graphs):
    """keep_gradients = False (the default): gs_adam_tf_step_zero_grad leaves the flat gradient cleared and the next run skips its fill
    pass (no fill inside the captured graphs either).  Same parameters, bit for bit, as the trainer that keeps the gradients and
    fills before every run; the buffers are all zeros after every step."""
    from gansynth_amd import variables
    out = {}
    for keep in (True, False):
        variables.set_default_store(variables.VariableStore(device="cuda"))
        pg, opg, model = make(1.0, variables.default_store(), full=False)
        model.keep_gradients, model.use_graphs = keep, graphs
        gp, dp = opg.init_params(seed=0, bias_std=0.1)
        for step in range(4):
            lat, lab, real = R.synthetic_batch(4, rank=step, image_shape=(2, 16, 128))
            if step == 0:
                model._build(cuda(lat), cuda(lab))
                variables.default_store().load_state_dict({**gp, **dp})
            model.discriminator_step(cuda(lat), cuda(lab), cuda(real))
            model.generator_step(cuda(lat), cuda(lab))
            if not keep:
                assert float(model.d_params.grad.abs().max()) == 0.0 and float(model.g_params.grad.abs().max()) == 0.0
                assert model.d_params.grad_clean and model.g_params.grad_clean
            else:
                assert float(model.d_params.grad.abs().max()) > 0.0 and float(model.g_params.grad.abs().max()) > 0.0
        out[keep] = (model.d_params.flat.clone(), model.g_params.flat.clone(), model.d_params.v.clone())
    # (two trainers in one process may associate the fp32 sums of multi-consumer gradients differently, see _same_up_to_accumulation_order)
    _same_up_to_accumulation_order(out[True][0], out[False][0], "discriminator parameters")
    _same_up_to_accumulation_order(out[True][1], out[False][1], "generator parameters")


def test_norm_backward_rides_in_the_data_gradient_convs_at_full_size(gpu_store):
    """BASELINE.json configs[1] shapes (batch 8, bf16, fully grown): in the generator run's plain backward the (leaky_relu -> pixel_norm)
    backward of the four 32- / 64-channel blocks runs inside the data-gradient conv of the block after them (three implicit-GEMM epilogues
    + the colour block's streaming pass) -- the calls are counted, their second-order addend is present, and the step equals the one with
    the fusion switched off (functional._FUSE_NORM_BWD) up to bf16 rounding of the one intermediate tensor the fused path never stores."""
    from gansynth_amd import functional as F, kernels, variables
    K = kernels.get()
    out = {}
    for fuse in (True, False):
        variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
        pg, opg, model = make(1.0, variables.default_store(), dtype=torch.bfloat16)
        lat, lab, _ = R.synthetic_batch(8, rank=0)
        c = lambda t: cuda(t).to(torch.bfloat16)
        model._build(c(lat), c(lab))
        calls = []
        orig_a, orig_b, was = K.conv2d_bwd_data_pnbwd, K.conv2d_transpose_bwd_data_pnbwd, F._FUSE_NORM_BWD
        K.conv2d_bwd_data_pnbwd = lambda *a, **k: (calls.append(("conv", a[2], k.get("addend") is not None)), orig_a(*a, **k))[1]
        K.conv2d_transpose_bwd_data_pnbwd = lambda *a, **k: (calls.append(("convT", tuple(a[3].shape), k.get("addend") is not None)), orig_b(*a, **k))[1]
        F._FUSE_NORM_BWD = fuse
        try:
            loss = float(model.generator_step(c(lat), c(lab)))
        finally:
            K.conv2d_bwd_data_pnbwd, K.conv2d_transpose_bwd_data_pnbwd, F._FUSE_NORM_BWD = orig_a, orig_b, was
        out[fuse] = (loss, {k: p.grad.clone() for k, p in model.g_params.named.items()}, calls)
    calls = out[True][2]
    assert out[False][2] == []
    shapes = sorted((kind, tuple(shape)[1:]) for kind, shape, _ in calls)
    assert shapes == [("conv", (32, 128, 1024)), ("conv", (32, 128, 1024)), ("conv", (64, 64, 512)), ("convT", (64, 64, 512))], shapes
    assert all(has_addend for _, _, has_addend in calls), calls   # the mode-seeking term's gradient into z reached every one of them
    assert abs(out[True][0] - out[False][0]) <= 1e-6 * max(1.0, abs(out[False][0]))   # (same forward)
    for k, g in out[False][1].items():
        if float(g.abs().max()) > 0:
            assert rel_l2(out[True][1][k], g) < 2e-2, (k, rel_l2(out[True][1][k], g))


def test_second_order_norm_kernels_ride_in_the_cotangent_convs_at_full_size(gpu_store):
    """Same shapes: in the second-order pass of the mode-seeking term (models.py:57-64) the convs run forward on cotangents, and where their
    tile owns all channels of a pixel both gradients of the block's (leaky_relu -> pixel_norm) backward node come out of the conv's epilogue
    (gs_conv_fwd_pnbwdbwd) -- the four 32- / 64-channel layers; counted, and the step equals the one with the fusion
    switched off (functional._FUSE_NORM_BWD2) up to bf16 rounding of the cotangent the fused path never stores."""
    from gansynth_amd import functional as F, kernels, variables
    K = kernels.get()
    out = {}
    for fuse in (True, False):
        variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
        pg, opg, model = make(1.0, variables.default_store(), dtype=torch.bfloat16)
        lat, lab, _ = R.synthetic_batch(8, rank=0)
        c = lambda t: cuda(t).to(torch.bfloat16)
        model._build(c(lat), c(lab))
        calls = []
        orig_a, orig_b, was = K.conv2d_fwd_pnbwdbwd, K.conv2d_transpose_fwd_pnbwdbwd, F._FUSE_NORM_BWD2
        K.conv2d_fwd_pnbwdbwd = lambda *a, **k: (calls.append(("conv", tuple(a[6].shape))), orig_a(*a, **k))[1]
        K.conv2d_transpose_fwd_pnbwdbwd = lambda *a, **k: (calls.append(("convT", tuple(a[4].shape))), orig_b(*a, **k))[1]
        F._FUSE_NORM_BWD2 = fuse
        try:
            loss = float(model.generator_step(c(lat), c(lab)))
        finally:
            K.conv2d_fwd_pnbwdbwd, K.conv2d_transpose_fwd_pnbwdbwd, F._FUSE_NORM_BWD2 = orig_a, orig_b, was
        out[fuse] = (loss, {k: p.grad.clone() for k, p in model.g_params.named.items()}, calls)
    assert out[False][2] == []
    shapes = sorted((kind, shape[1:]) for kind, shape in out[True][2])
    assert shapes == [("conv", (32, 128, 1024)), ("conv", (64, 64, 512)), ("convT", (32, 128, 1024)), ("convT", (64, 64, 512))], shapes
    assert abs(out[True][0] - out[False][0]) <= 1e-6 * max(1.0, abs(out[False][0]))
    for k, g in out[False][1].items():
        if float(g.abs().max()) > 0:
            assert rel_l2(out[True][1][k], g) < 2e-2, (k, rel_l2(out[True][1][k], g))


@pytest.mark.parametrize("full,dtype", [(False, torch.float32), (True, torch.bfloat16)])
def test_discriminator_tail_over_real_and_fake_as_one_batch(gpu_store, full, dtype):
    """The discriminator run sends [real; fake] through the network's latency-bound tail as ONE batch (models.GANSynth._d_losses_b_batched:
    trunk per batch, networks.PGGAN.discriminator_tail with the minibatch statistic per half, the R1 seed on the real rows, the one-launch
    loss on the stacked logits).  Same loss and the same gradient for every discriminator parameter as with the two separate passes
    (models._BATCH_D_TAIL off) -- fp32 on the reduced network to accumulation-order accuracy, bf16 at full size to bf16 rounding of the
    few tensors whose summation order changes (the weight gradients of the tail now sum 16 images in one source instead of 8 + 8)."""
    from gansynth_amd import models, variables
    out = {}
    for batched in (True, False):
        variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
        pg, opg, model = make(1.0, variables.default_store(), full=full, dtype=dtype)
        shape = (2, 128, 1024) if full else (2, 16, 128)
        lat, lab, real = R.synthetic_batch(8, rank=0, image_shape=shape)
        c = lambda t: cuda(t).to(dtype)
        model._build(c(lat), c(lab))
        model.batch_d_tail = batched   # (default: batched unless the runs fork, models.GANSynth._batched_tail)
        assert model._batched_tail(True, c(real)) == batched
        loss = float(model.discriminator_step(c(lat), c(lab), c(real)))
        out[batched] = (loss, {k: p.grad.clone() for k, p in model.d_params.named.items()})
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert abs(out[True][0] - out[False][0]) <= (1e-6 if dtype == torch.float32 else 2e-3) * max(1.0, abs(out[False][0])), (out[True][0], out[False][0])
    compared = 0
    for k, g in out[False][1].items():
        if float(g.abs().max()) > 0:   # (the colour blocks of the levels below the head take no part in a fully grown pass)
            compared += 1
            assert rel_l2(out[True][1][k], g) < tol, (k, rel_l2(out[True][1][k], g))
        else:
            assert float(out[True][1][k].abs().max()) == 0, k
    assert compared >= 14


def test_training_driver_visits_every_growing_regime_and_resumes(gpu_store, tmp_path):
    """BASELINE.json config 5 at reduced size: GANSynth.train with the reference's loop semantics (models.py:110-194) -- generated
    notes -> HIP spectral front end -> real images, growing_level = global_step / growing_steps walking from the 2x16 stage through
    every fade-in to the fully grown networks (where the step switches to hipGraph replay), checkpoints under the TF variable
    names, and a second trainer that resumes from them."""
    from gansynth_amd import checkpoint, variables
    from gansynth_amd.dataset import synthetic_nsynth_input_fn
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict

    growing_steps, total = 24, 16
    spectral = Dict(waveform_length=1024, sample_rate=16000, spectrogram_shape=[16, 128], overlap=0.75)

    def make(seed):
        variables.set_default_store(variables.VariableStore(device="cuda", seed=seed))
        holder = {}
        pg = PGGAN(min_resolution=[2, 16], max_resolution=[16, 128], min_channels=32, max_channels=64,
                   growing_level=lambda: holder["m"].global_step / growing_steps)
        notes = synthetic_nsynth_input_fn(4, range(24, 85), device="cuda", seed=7)

        def real_input_fn():
            wav, lab = notes()
            return wav[:, :1024].contiguous(), lab

        gen = torch.Generator(device="cuda").manual_seed(11)
        m = GANSynth(pg.generator, pg.discriminator, real_input_fn, lambda: torch.randn(4, 256, device="cuda", generator=gen), spectral,
                     Dict(R.DEFAULT_HYPER), use_graphs=True)
        holder["m"] = m
        return m, pg

    logs = []
    model, pg = make(0)
    depths = []
    orig = model.train_step

    def step():
        depths.append(pg.growing_depth)
        return orig()

    model.train_step = step
    model.train(total_steps=total, log_tensor_steps=4, log=logs.append, model_dir=str(tmp_path), save_checkpoint_steps=8)
    assert model.global_step == total and len(logs) == total // 4 and all("generator_loss" in l for l in logs)
    assert depths[0] == 0.0 and any(0.0 < d < 1.0 for d in depths) and any(1.0 < d < 2.0 for d in depths) and any(2.0 < d < 3.0 for d in depths)
    assert depths[-1] > 3.0 and replaying_graphs(model)            # fully grown at the end: replaying graphs
    assert torch.isfinite(model.g_params.flat).all() and torch.isfinite(model.d_params.flat).all()
    assert np.isfinite(float(model.discriminator_loss)) and np.isfinite(float(model.generator_loss))
    assert checkpoint.latest(str(tmp_path)).endswith(f"model.ckpt-{total}.safetensors")
    # resume: everything comes from the file; two more iterations run (fully grown from the first step on)
    again, _ = make(99)
    again.train(total_steps=total + 2, log=None, model_dir=str(tmp_path), save_checkpoint_steps=0)
    assert again.restored_from.endswith(f"model.ckpt-{total}.safetensors") and again.global_step == total + 2
    assert again.d_params.t == total + 2 and torch.isfinite(again.g_params.flat).all()
    # generate (models.py:232-250): waveforms of the configured length in [-1, 1]-ish range
    lat = torch.randn(4, 256, device="cuda")
    lab = torch.nn.functional.one_hot(torch.randint(0, 61, (4,)), 61).float().cuda()
    wav = again.generate(lat, lab)
    assert tuple(wav.shape) == (4, 1024) and torch.isfinite(wav).all()


@pytest.mark.parametrize("graphs", [False, True])
def test_train_trajectory_vs_oracle(graphs):
    """The training driver against the oracle over SEVERAL iterations (models.py:189-194: per iteration one discriminator run and one
    generator run on fresh batches, `global_step` bumped by the generator run only, growing_level = global_step / growing_steps,
    gan_synth_main.py:51-54): six iterations of GANSynth.train() on the reduced PGGAN with growing_steps = 40, i.e. iteration 0 at the
    2x16 stage, iterations 1-2 in the first fade-in, 3-5 in the second (two regime changes; with `graphs` each regime is captured
    and replayed, the fade weight read from device memory), against oracle.torch_ref.Trainer driven by the same batches in the same
    order.  Per iteration: both losses at 1e-3, global_step and growing_depth exact; at the end every parameter's accumulated
    UPDATE (p_final - p_initial, six TF-Adam steps with carried m / v) at 1e-2 relative L2, untaken branches exactly unmoved."""
    from gansynth_amd import variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict
    growing_steps, total = 40, 6
    kw = dict(min_resolution=[2, 16], max_resolution=[16, 128], min_channels=32, max_channels=64)
    variables.set_default_store(variables.VariableStore(device="cuda"))
    holder = {}
    pg = PGGAN(growing_level=lambda: holder["m"].global_step / growing_steps, **kw)
    opg = R.PGGAN(growing_level=lambda: holder["t"].global_step / growing_steps, **kw)
    batches = [R.synthetic_batch(4, rank=i, image_shape=(2, 16, 128)) for i in range(2 * total)]   # (latents, labels, real images)
    calls = {"real": 0, "fake": 0}

    def real_input_fn():   # D run: images + labels of batch 2i; G run: the labels of batch 2i + 1 (models.GANSynth._next_inputs)
        _, lab, real = batches[calls["real"]]
        calls["real"] += 1
        return cuda(real), cuda(lab)

    def fake_input_fn():
        lat = batches[calls["fake"]][0]
        calls["fake"] += 1
        return cuda(lat)

    model = GANSynth(pg.generator, pg.discriminator, real_input_fn, fake_input_fn, None, Dict(R.DEFAULT_HYPER), use_graphs=graphs)
    holder["m"] = model
    gp, dp = opg.init_params(seed=0, bias_std=0.1)
    model._build(cuda(batches[0][0]), cuda(batches[0][1]))
    variables.default_store().load_state_dict({**gp, **dp})
    tr = holder["t"] = R.Trainer(opg, gp, dp)
    trace, orig = [], model.train_step

    def step():
        depth = pg.growing_depth
        d_loss, g_loss = orig()
        trace.append((depth, float(d_loss), float(g_loss), model.global_step))
        return d_loss, g_loss

    model.train_step = step
    model.train(total_steps=total, log=None)
    assert model.global_step == total and len(trace) == total and calls == {"real": 2 * total, "fake": 2 * total}
    regimes = []
    for i in range(total):
        depth = opg.growing_depth
        head = pg._head_depth(depth)
        if not regimes or regimes[-1] != (head[0], head[1] is not None):
            regimes.append((head[0], head[1] is not None))
        od, _ = tr.d_step(batches[2 * i][0], batches[2 * i][1], batches[2 * i][2])
        og, _ = tr.g_step(batches[2 * i + 1][0], batches[2 * i + 1][1])
        h_depth, h_d, h_g, h_step = trace[i]
        assert h_depth == depth and h_step == tr.global_step == i + 1, (i, h_depth, depth, h_step)
        assert abs(h_d - float(od)) <= 1e-3 * max(1.0, abs(float(od))), f"iteration {i}: discriminator loss {h_d} vs oracle {float(od)}"
        assert abs(h_g - float(og)) <= 1e-3 * max(1.0, abs(float(og))), f"iteration {i}: generator loss {h_g} vs oracle {float(og)}"
    assert regimes == [(0, False), (1, True), (2, True)], regimes
    assert model.d_params.t == tr.d_t == total and model.g_params.t == tr.g_t == total
    worst = 0.0
    for params, init, final in ((model.d_params, dp, tr.d), (model.g_params, gp, tr.g)):
        for k, p in params.named.items():
            ref = (final[k].detach() - init[k]).double()
            upd = (p.data.cpu() - init[k]).double()
            if float(ref.abs().max()) == 0.0:
                assert float(upd.abs().max()) == 0.0, k   # a block no regime reached: untouched by six Adam steps
                continue
            err = float((upd - ref).norm() / ref.norm())
            worst = max(worst, err)
            assert err < 1e-2, f"{k}: accumulated update differs by {err:.3e} (relative L2)"
    print(f"trajectory ({'graphs' if graphs else 'eager'}): worst accumulated-update error {worst:.2e}")
    if graphs:
        assert replaying_graphs(model, (2, False))


def test_generate_vs_oracle(gpu_store):
    """models.py:232-250 end to end: latents + labels -> generator -> (log-mel, IF) images -> waveforms, the HIP path (MFMA convs,
    gs_mel_if_to_waveform) against the oracle (torch-CPU generator + numpy inverse) on the same parameters.  1e-3 of the peak is
    the contract; the phases are a cumulative sum over the frames, so image differences of 1e-5 arrive as ~1e-4."""
    from gansynth_amd.utils import Dict
    from oracle import spectral_np as S
    pg, opg, model = make(1.0, gpu_store, full=False)
    lat, lab, _ = R.synthetic_batch(4, rank=0)
    gp, dp = opg.init_params(seed=3, bias_std=0.1)
    model._build(cuda(lat), cuda(lab))
    gpu_store.load_state_dict({**gp, **dp})
    P = dict(waveform_length=1024, sample_rate=16000, spectrogram_shape=[16, 128], overlap=0.75)
    model.spectral_params = Dict(P)
    wav = model.generate(cuda(lat), cuda(lab)).cpu().numpy()
    with torch.no_grad():
        img = opg.generator(gp, lat, lab).numpy()
    ref = S.convert_to_waveform(img[:, 0], img[:, 1], **P)
    assert wav.shape == ref.shape == (4, 1024)
    for a, b in zip(wav, ref):
        scale = np.abs(b).max()
        assert scale > 0 and np.abs(a - b).max() / scale < 1e-3, np.abs(a - b).max() / scale
        assert S.cross_correlation(a, b) > 0.99999


def test_hipgraph_replay_in_a_fade_in_regime(gpu_store):
    """Graphs are captured in every growing regime: the fade-in weight is read from device memory (gs_axpby_dev), so the replayed
    step follows a growing_level that changes every iteration; a regime change re-captures.  Same losses / parameters as eager
    launches (up to the order of fp32 gradient accumulation)."""
    from gansynth_amd import variables
    out = {}
    for graphs in (False, True):
        variables.set_default_store(variables.VariableStore(device="cuda"))
        step = [0]
        pg, opg, model = make(lambda: 0.20 + 0.03 * step[0], variables.default_store(), full=False)   # depth 2.0 .. 2.5 .. 3.1 of 3
        model.use_graphs = graphs
        gp, dp = opg.init_params(seed=0, bias_std=0.1)
        losses, keys = [], []
        for it in range(7):
            step[0] = it
            lat, lab, real = R.synthetic_batch(4, rank=it, image_shape=(2, 16, 128))
            if it == 0:
                model._build(cuda(lat), cuda(lab))
                variables.default_store().load_state_dict({**gp, **dp})
            losses.append(float(model.discriminator_step(cuda(lat), cuda(lab), cuda(real))))
            losses.append(float(model.generator_step(cuda(lat), cuda(lab))))
            keys.append(model._graph_key)
        out[graphs] = (losses, model.d_params.flat.clone(), model.g_params.flat.clone())
        if graphs:
            assert set(model._graphs) == {"d", "g"} and pg.fade_weight is None
            assert len(set(keys)) >= 2 and keys[0][1] is False     # started inside a fade-in, crossed into the next regime
    for i, (a, b) in enumerate(zip(out[False][0], out[True][0])):
        _same_up_to_accumulation_order(a, b, f"loss {i}")
    _same_up_to_accumulation_order(out[False][1], out[True][1], "discriminator parameters")
    _same_up_to_accumulation_order(out[False][2], out[True][2], "generator parameters")


@pytest.mark.parametrize("level", [1.0, 0.6])
def test_discriminator_gradient_all_reduced_in_two_steps(level):
    """models.GANSynth._arm_first_bucket (data parallel, one graph per iteration; world size 1 on the library's RCCL communicator): the layers of the
    lower pyramid are complete long before the backward ends (kernels.complete_rule counts their pairs against the previous pass), their
    contraction runs on the branch and the part of the flat gradient that holds none of the other layers' gradients -- 98 % of it at
    BASELINE.json configs[1] -- goes on the wire behind it, beside the rest of the backward; the two ends follow behind the final contraction.
    Same gradients as the one-message form up to the association of the regrouped contractions (both learning rates at zero, so that nothing
    amplifies a last bit: the gradient buffers of three iterations), the first message covers the range it should; the iteration time with
    300-us stand-ins for the collectives is reported for both forms.  Level 0.6: the same in a fade-in regime (two colour blocks, a smaller
    network: whatever the lower pyramid is there goes first; gradients only)."""
    import time
    import torch.distributed as dist
    from gansynth_amd.utils import Dict
    hyper = Dict(R.DEFAULT_HYPER)
    hyper.generator_learning_rate = hyper.discriminator_learning_rate = 0.0
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % (29400 + os.getpid() % 500), rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        batches = [R.synthetic_batch(8, rank=i, image_shape=(2, 128, 1024)) for i in range(2)]
        out, ms = {}, {}
        for two_step in (True, False):
            model = _dp_trainer(level, batches, full=True, dtype=torch.bfloat16, keep=True, hyper=hyper)
            model.bucket_d_reduce = two_step
            losses, grads = [], []
            for _ in range(3):
                losses.append(tuple(float(x) for x in model.train_step()))
                model.synchronize()
                grads.append((model.d_params.grad.clone(), model.g_params.grad.clone()))
            out[two_step] = (losses, grads, None, model.first_bucket, bool(model._merged and model._merged.get("fused")))
            total = model.d_params.grad.numel()
            names = list(model.d_params.named.items())
            if two_step:
                lo, hi = model.first_bucket
                base = model.d_params.grad.data_ptr()
                inside = [n for n, p in names if lo <= (p.grad.data_ptr() - base) // 4 and (p.grad.data_ptr() - base) // 4 + p.numel() <= hi]
            model._comm.set_marker_us(300.0)   # (stand-ins are read when a launch is captured: new graphs)
            model._merged = None
            model._graphs.clear()
            for _ in range(3):
                model.train_step()
            model.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                model.train_step()
            model.synchronize()
            ms[two_step] = (time.perf_counter() - t0) / 20 * 1e3
            model._comm.set_marker_us(-1.0)
            del model
        assert out[True][4] and out[False][4], "one graph per iteration expected"
        assert out[False][3] is None and out[True][3] is not None
        lo, hi = out[True][3]
        assert any("conv_block_2x16/dense/weight" in n for n in inside), inside
        if level == 1.0:
            assert hi - lo > 0.9 * total, (lo, hi, total)
            assert any("conv_block_16x128/conv/weight" in n for n in inside)
            assert not any(("128x1024" in n or "conv_block_64x512" in n) for n in inside), inside
        assert out[True][0] == out[False][0], (out[True][0], out[False][0])   # (the weights never move: the forward passes are the same launches)
        for it, (ga, gb) in enumerate(zip(out[True][1], out[False][1])):
            for k, name in ((0, "discriminator"), (1, "generator")):
                err = float((ga[k] - gb[k]).abs().max()) / float(gb[k].abs().max())
                assert err <= 2e-5, (it, name, err)   # (fp32 sums of the same bf16 products, grouped differently)
            assert torch.equal(ga[1], gb[1]), "the generator run's launches do not change"
        print("level %s: first message %s of %d floats; ms per iteration with 300-us stand-ins: two steps %.3f, one message %.3f"
              % (level, out[True][3], total, ms[True], ms[False]))
        # (what the stand-ins cost is REPORTED, not asserted: fully grown 5.92 against 6.05 ms in one process, 5.87 against 5.89 in another -- which
        #  chains of a replayed graph share a hardware queue depends on the stream pool's history -- and in the fade-in regime 6.24 against 6.09:
        #  the form is opt-in)
    finally:
        dist.destroy_process_group()


def test_distributed_step_on_rccl_world_size_1():
    """The data-parallel path on the real collective backend: torch.distributed backend "nccl" (= RCCL on ROCm) with ONE rank --
    the only world size this box has.  Bucketed gradient all-reduce (16 KiB buckets: many collectives per run, launched from the
    backward's tail in eager mode, behind the graph replay otherwise), TF-Adam bucket by bucket.  With one rank the sum is the
    identity and the averaging factor 1, so losses and parameters must equal the non-distributed step's, eager and replayed.  The
    collectives go through libgansynth_hip.so's own communicator (gs_comm_*, RCCL on the backward's stream) and, with
    GS_TORCH_COLLECTIVES=1, through torch.distributed's."""
    import torch.distributed as dist
    from gansynth_amd import variables
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % (29400 + os.getpid() % 500), rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        out = {}
        for mode in ("plain", "dist", "dist+graphs", "dist+graphs, collective refused by the capture", "dist+torch"):
            variables.set_default_store(variables.VariableStore(device="cuda"))
            pg, opg, model = make(1.0, variables.default_store(), full=False)
            model.distributed, model.world, model.bucket_bytes = mode != "plain", 1, 16 << 10
            if mode == "dist+torch":
                os.environ["GS_TORCH_COLLECTIVES"] = "1"
            else:
                os.environ.pop("GS_TORCH_COLLECTIVES", None)
            if "refused" in mode:   # the all-reduce raises under stream capture: the run is captured again without it and reduced eagerly
                def refuse(params):
                    raise RuntimeError("simulated failure of a collective under stream capture")
                model._reduce_in_capture = refuse
            model.use_graphs = mode.startswith("dist+graphs")
            gp, dp = opg.init_params(seed=0, bias_std=0.1)
            losses = []
            for step in range(3):
                lat, lab, real = R.synthetic_batch(4, rank=step, image_shape=(2, 16, 128))
                if step == 0:
                    model._build(cuda(lat), cuda(lab))
                    variables.default_store().load_state_dict({**gp, **dp})
                losses.append(float(model.discriminator_step(cuda(lat), cuda(lab), cuda(real))))
                losses.append(float(model.generator_step(cuda(lat), cuda(lab))))
            torch.cuda.synchronize()
            out[mode] = (losses, model.d_params.flat.clone(), model.g_params.flat.clone(), len(model.g_params.buckets), model._comm is not None,
                         model._graph_allreduce, model._run_reduced)
        assert out["plain"][3] == 1 and out["dist"][3] > 4
        assert model._comm is None and out["dist"][4] and out["dist+graphs"][4]
        assert out["dist+graphs"][5] and out["dist+graphs"][6]   # the replayed graph carried the all-reduce ...
        refused = out["dist+graphs, collective refused by the capture"]
        assert refused[4] and not refused[5] and not refused[6]   # ... and here it did not: reduced eagerly behind every replay
        for mode in ("dist", "dist+graphs", "dist+graphs, collective refused by the capture", "dist+torch"):   # (two trainers in one process may associate fp32 gradient sums differently, see above)
            for i, (a, b) in enumerate(zip(out["plain"][0], out[mode][0])):
                _same_up_to_accumulation_order(a, b, f"{mode}: loss {i}")
            # (torch.distributed's transport keeps round 4's schedule -- real and fake batch through the discriminator's tail as ONE batch, no early
            #  contraction: other launches, other association from the first gradient on (6e-9 of its scale), and after three TF-Adam steps a tenth
            #  of the generator's elements are more than 1e-5 apart, scripts/dbg_dist_torch.py; the three modes on the library's own communicator
            #  issue the plain schedule's launches and are BIT-identical to it since the engine's node order is process-wide, functional._NODE_SEQ)
            far = 0.3 if mode == "dist+torch" else 2e-2
            _same_up_to_accumulation_order(out["plain"][1], out[mode][1], f"{mode}: discriminator parameters", far_fraction=far)
            _same_up_to_accumulation_order(out["plain"][2], out[mode][2], f"{mode}: generator parameters", far_fraction=far)
        for mode in ("dist", "dist+graphs"):
            assert torch.equal(out["plain"][1], out[mode][1]) and torch.equal(out["plain"][2], out[mode][2]), mode
    finally:
        os.environ.pop("GS_TORCH_COLLECTIVES", None)
        dist.destroy_process_group()


@pytest.mark.parametrize("level,full", [(1.0, False), (0.6, False), (1.0, True)])
def test_one_bit_masks_change_nothing_in_the_iteration(gpu_store, level, full, monkeypatch):
    """kernels._MASK_BITS (GS_NO_MASK_BITS): the discriminator's leaky-relu results carry their sign words and the masked launches read them -- or
    read the values.  Same launches otherwise, same order: losses, gradients and parameters of two bf16 iterations (eager; reduced size fully
    grown and in a fade-in, and BASELINE.json configs[1] itself) are the same bit for bit, and the sign words really were in play."""
    from gansynth_amd import kernels, variables
    dtype = torch.bfloat16
    n = 8 if full else 4
    res = (2, 128, 1024) if full else (2, 16, 128)
    batches = [R.synthetic_batch(n, rank=i, image_shape=res) for i in range(2)]
    out, used = {}, {}
    for mode in (True, False):
        monkeypatch.setattr(kernels, "_MASK_BITS", mode)
        seen = []
        real_mask_act = kernels._mask_act
        monkeypatch.setattr(kernels, "_mask_act", lambda m, a, f=real_mask_act: (seen.append(f(m, a)), seen[-1])[1])
        variables.set_default_store(variables.VariableStore(device="cuda"))
        pg, opg, model = make(level, variables.default_store(), full=full, dtype=dtype)
        model.use_graphs = False
        gp, dp = opg.init_params(seed=0, bias_std=0.1)
        rec = []
        for step, (lat, lab, real) in enumerate(batches):
            lat, lab, real = cuda(lat).to(dtype), cuda(lab).to(dtype), cuda(real).to(dtype)
            if step == 0:
                model._build(lat, lab)
                variables.default_store().load_state_dict({**gp, **dp})
            rec.append(model.discriminator_step(lat, lab, real).clone())
            rec.append(model.d_params.grad.clone())
            rec.append(model.generator_step(lat, lab).clone())
            rec.append(model.g_params.grad.clone())
        torch.cuda.synchronize()
        rec += [model.d_params.flat.clone(), model.g_params.flat.clone()]
        out[mode], used[mode] = rec, seen
        monkeypatch.setattr(kernels, "_mask_act", real_mask_act)
        del model
    from gansynth_amd import _lib
    assert used[True] and all(a == _lib.ACT_LRELU_BITS for a in used[True]), sorted(set(used[True]))
    assert used[False] and _lib.ACT_LRELU_BITS not in used[False]
    assert len(used[True]) == len(used[False])
    for i, (a, b) in enumerate(zip(out[True], out[False])):
        assert torch.equal(a, b), f"record {i}: sign words and values disagree"


@pytest.mark.parametrize("level,full,dtype", [(1.0, False, torch.float32), (0.6, False, torch.float32), (1.0, True, torch.bfloat16)])
def test_forked_branches_change_nothing_but_the_schedule(gpu_store, level, full, dtype):
    """models.GANSynth._branch: inside a run's hipGraph the discriminator's pass over G(z) (forward, and through autograd its backward) runs
    beside the generator's mode-seeking passes, the whole fake pass of the discriminator run beside the real one with its R1 passes, and the weight
    gradients of the full-chip levels beside the few-block chain of the backward below them (kernels.early_flush_rule) -- on a forked
    branch of the graph.  The host-side launch order is the same with and without branches, so losses and parameters after three iterations
    are the same bit for bit (reduced size fully grown / fade-in, and BASELINE.json configs[1] itself: full size, bf16, batch 8); the same
    branches with eager launches (two streams, events) agree as well."""
    from gansynth_amd import variables
    out = {}
    n = 8 if full else 4
    res = (2, 128, 1024) if full else (2, 16, 128)
    batches = [R.synthetic_batch(n, rank=i, image_shape=res) for i in range(3)]
    for mode in ("plain", "forked", "forked-eager"):
        variables.set_default_store(variables.VariableStore(device="cuda"))
        pg, opg, model = make(level, variables.default_store(), full=full, dtype=dtype)
        model.use_graphs = mode != "forked-eager"
        model.fork = mode != "plain"
        model.fork_eager = mode == "forked-eager"
        model.early_flush_always = True   # (the plain schedule contracts the large layers at the same points of its launch sequence, in place)
        model.batch_d_tail = False        # (and keeps the real and the fake pass of the discriminator run apart, as the forked one does)
        gp, dp = opg.init_params(seed=0, bias_std=0.1)
        losses = []
        for step, (lat, lab, real) in enumerate(batches):
            lat, lab, real = cuda(lat).to(dtype), cuda(lab).to(dtype), cuda(real).to(dtype)
            if step == 0:
                model._build(lat, lab)
                variables.default_store().load_state_dict({**gp, **dp})
            losses.append(float(model.discriminator_step(lat, lab, real)))
            losses.append(float(model.generator_step(lat, lab)))
        torch.cuda.synchronize()
        out[mode] = (losses, model.d_params.flat.clone(), model.g_params.flat.clone(), model.branches_opened)
        del model
    assert out["plain"][3] == 0
    assert out["forked"][3] == 4, out["forked"][3]           # per captured run: the independent sub-pass and the early weight gradients
    assert out["forked-eager"][3] == 4 * len(batches)
    for mode in ("forked", "forked-eager"):
        for i, (a, b) in enumerate(zip(out["plain"][0], out[mode][0])):
            _same_up_to_accumulation_order(a, b, f"{mode}: loss {i}")
        # (three iterations: an element that stepped the other way in the first one moves every later gradient by ~1e-3 and more elements follow --
        #  0.3 % of the discriminator's after the third when this test runs alone in a fresh process, none inside the suite; the CAPTURED forked
        #  schedule is held to bit-identity below)
        _same_up_to_accumulation_order(out["plain"][1], out[mode][1], f"{mode}: discriminator parameters")
        _same_up_to_accumulation_order(out["plain"][2], out[mode][2], f"{mode}: generator parameters")
    same = [bool(torch.equal(out["plain"][k], out["forked"][k])) for k in (1, 2)]
    print("forked graphs vs plain graphs bit-identical (D, G):", same, "losses:", out["plain"][0], out["forked"][0])
    assert all(same), same


@pytest.mark.parametrize("level,full,dtype", [(1.0, False, torch.float32), (0.6, False, torch.float32), (1.0, True, torch.bfloat16)])
def test_generator_part_a_inside_the_discriminator_graph(gpu_store, level, full, dtype):
    """models.GANSynth._train_step_merged: train_step() on one GPU with graphs captures part A of the generator run (G(z) and the mode-seeking
    first-order pass) inside the discriminator run's graph, on a stream of its own from the graph's root.  Same launches on the same operands as
    the two runs one after the other: losses and parameters after four iterations agree with the unmerged schedule (to the association of
    multi-consumer gradient sums, see _same_up_to_accumulation_order; bit-identity is reported), in a fade-in regime and fully grown, reduced
    size and configs[1] itself."""
    from gansynth_amd import variables
    out = {}
    n = 8 if full else 4
    res = (2, 128, 1024) if full else (2, 16, 128)
    batches = [R.synthetic_batch(n, rank=i, image_shape=res) for i in range(4)]
    for merged in (False, "pair", "one graph"):
        variables.set_default_store(variables.VariableStore(device="cuda"))
        pg, opg, model = make(level, variables.default_store(), full=full, dtype=dtype)
        model.use_graphs, model.keep_gradients = True, False
        model.merge_runs = bool(merged)
        model.fuse_iteration = merged == "one graph"   # (round 6: the whole iteration ONE graph, both optimizer steps inside)
        cur = [0]

        def real_input_fn():
            lat, lab, real = batches[cur[0] % len(batches)]
            return cuda(real).to(dtype), cuda(lab).to(dtype)

        def fake_input_fn():
            lat, _, _ = batches[cur[0] % len(batches)]
            cur[0] += 1
            return cuda(lat).to(dtype)
        model.real_input_fn, model.fake_input_fn = real_input_fn, fake_input_fn
        gp, dp = opg.init_params(seed=0, bias_std=0.1)
        lat, lab, _ = batches[0]
        model._build(cuda(lat).to(dtype), cuda(lab).to(dtype))
        variables.default_store().load_state_dict({**gp, **dp})
        losses = []
        for _ in range(4):
            d_loss, g_loss = model.train_step()
            losses += [float(d_loss), float(g_loss)]
        assert (model._merged is not None) == bool(merged) and model.global_step == 4
        if merged == "one graph":   # the generator's fourth step is pending: it rides at the front of the NEXT replay -- or is applied here
            assert model._merged["fused"] and model._merged["y"] is None and model._g_pending is not None
            assert (model.d_params.t, model.g_params.t) == (4, 4)
        else:
            assert model._g_pending is None
        model.synchronize()
        assert model._g_pending is None
        out[merged] = (losses, model.d_params.flat.clone(), model.g_params.flat.clone())
        if merged == "one graph":   # ... and a plain run afterwards finds nothing pending and a clean gradient buffer
            lat, lab, real = batches[1]
            assert np.isfinite(float(model.discriminator_step(cuda(lat).to(dtype), cuda(lab).to(dtype), cuda(real).to(dtype))))
            model.train_step()      # (back on the one-graph path: recaptured or replayed, nothing pending at its front)
            model.synchronize()
            assert model.global_step == 5 and bool(torch.isfinite(model.g_params.flat).all())
        del model
    for mode in ("pair", "one graph"):
        for i, (a, b) in enumerate(zip(out[False][0], out[mode][0])):
            _same_up_to_accumulation_order(a, b, f"{mode}: loss {i}")
        _same_up_to_accumulation_order(out[False][1], out[mode][1], f"{mode}: discriminator parameters")
        _same_up_to_accumulation_order(out[False][2], out[mode][2], f"{mode}: generator parameters")
        print(mode, "vs two runs bit-identical (D, G):", [bool(torch.equal(out[False][k], out[mode][k])) for k in (1, 2)])
    # the one graph holds the same launches on the same operands as the pair: only lr_t travels differently (device memory instead of by value)
    same = [bool(torch.equal(out["pair"][k], out["one graph"][k])) for k in (1, 2)]
    print("one graph vs pair bit-identical (D, G):", same)
    assert out["pair"][0] == out["one graph"][0] and all(same), (same, out["pair"][0], out["one graph"][0])


@pytest.mark.parametrize("full,dtype,iterations", [(False, torch.float32, 240), (False, torch.bfloat16, 240), (True, torch.bfloat16, 45)])
def test_replayed_iterations_reproduce_the_eager_gradients(gpu_store, full, dtype, iterations):
    """A missing dependency between two streams of a captured iteration shows as a WRONG NUMBER ONCE IN A WHILE, which comparisons after a few
    optimizer steps cannot tell from TF-Adam's amplification of round-off.  Here both learning rates are zero: the parameters never move, every
    replayed iteration must reproduce the eagerly launched, one-stream gradients of its batch (three batches in rotation), and hundreds of
    replays are checked one by one -- every schedule (one graph, the pair, no branches), reduced size fp32 / bf16 and configs[1] itself.
    (Round 6: this found the real and the fake pass's `_WeightSlice.backward` adding into one slice of w.grad from two streams unordered --
    one contribution lost in ~2 % of the fp32 iterations.)"""
    from gansynth_amd import variables
    from gansynth_amd.utils import Dict
    n, res = (8, (2, 128, 1024)) if full else (4, (2, 16, 128))
    batches = [R.synthetic_batch(n, rank=i, image_shape=res) for i in range(3)]
    hyper = Dict(R.DEFAULT_HYPER)
    hyper.generator_learning_rate = hyper.discriminator_learning_rate = 0.0
    tol = 1e-5 if dtype == torch.float32 else 1e-3   # (same kernels on the same operands: association of fp32 sums only)
    ref = None
    for mode in ("eager", "one graph", "pair", "no branches"):
        variables.set_default_store(variables.VariableStore(device="cuda"))
        pg, opg, model = make(1.0, variables.default_store(), full=full, dtype=dtype, hyper=hyper)
        model.use_graphs, model.keep_gradients = mode != "eager", True
        model.fuse_iteration = mode != "pair"
        if mode == "no branches":
            model.fork = False
        cur = [0]

        def real_input_fn():
            lat, lab, real = batches[cur[0] % 3]
            return cuda(real).to(dtype), cuda(lab).to(dtype)

        def fake_input_fn():
            lat, _, _ = batches[cur[0] % 3]
            cur[0] += 1
            return cuda(lat).to(dtype)
        model.real_input_fn, model.fake_input_fn = real_input_fn, fake_input_fn
        gp, dp = opg.init_params(seed=0, bias_std=0.1)
        lat, lab, _ = batches[0]
        model._build(cuda(lat).to(dtype), cuda(lab).to(dtype))
        variables.default_store().load_state_dict({**gp, **dp})
        rec, wrong = [], []
        for it in range(3 if mode == "eager" else (iterations if mode in ("one graph", "pair") else iterations // 3)):
            model.train_step()
            model.synchronize()
            grads = (model.d_params.grad.clone(), model.g_params.grad.clone())
            if mode == "eager":
                rec.append(grads)
                continue
            for k, what in ((0, "discriminator"), (1, "generator")):
                err = float((grads[k] - ref[it % 3][k]).abs().max()) / float(ref[it % 3][k].abs().max())
                if not err <= tol:
                    wrong.append((it, what, err))
        if mode == "eager":
            ref = rec
        else:
            assert not wrong, (mode, len(wrong), wrong[:6])
        del model


def _dp_trainer(level, batches, full=False, dtype=torch.float32, distributed=True, graphs=True, keep=True, hyper=None):
    from gansynth_amd import variables
    variables.set_default_store(variables.VariableStore(device="cuda"))
    pg, opg, model = make(level, variables.default_store(), full=full, dtype=dtype, hyper=hyper)
    model.keep_gradients = keep
    model.distributed, model.world, model.use_graphs = distributed, 1, graphs
    cur = [0]

    def real_input_fn():
        lat, lab, real = batches[cur[0] % len(batches)]
        return cuda(real).to(dtype), cuda(lab).to(dtype)

    def fake_input_fn():
        lat, _, _ = batches[cur[0] % len(batches)]
        cur[0] += 1
        return cuda(lat).to(dtype)

    model.real_input_fn, model.fake_input_fn = real_input_fn, fake_input_fn
    gp, dp = opg.init_params(seed=0, bias_std=0.1)
    lat, lab, _ = batches[0]
    model._build(cuda(lat).to(dtype), cuda(lab).to(dtype))
    variables.default_store().load_state_dict({**gp, **dp})
    return model


def test_gradient_all_reduce_rides_in_the_part_a_graph_of_the_other_run():
    """the all-reduce overlapped with compute.  Data parallel with graphs, train_step() runs every run as two
    graphs and the all-reduce of the OTHER network's flat gradient is a forked branch of the part-A graph (models.GANSynth.
    _capture_pair).  On the one rank this box has: (i) parameters after 4 iterations are bit-identical to the serial data-parallel
    form (all-reduce as the last node of each run's graph, GS_NO_OVERLAP_REDUCE) in a fade-in regime and fully grown, with the
    zeroing and the gradient-keeping optimizer step; a pending generator update is flushed by synchronize(); (ii) a capture failure
    of the collective on ANY rank takes every rank to the eager form together (the agreement all-reduce is exercised with world 1);
    (iii) WHERE the collective sits: RCCL short-cuts a one-rank all-reduce to nothing, so GS_COMM_MARKER_US puts a 1-block kernel
    that holds its stream for 300 us in its place -- beside part A it must not lengthen the full-size iteration, on the critical path
    (the serial form) it adds two of them."""
    import time
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % (29400 + (os.getpid() + 7) % 500), rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        os.environ.pop("GS_COMM_MARKER_US", None)
        for level, keep in ((1.0, True), (1.0, False), (0.25, False)):
            batches = [R.synthetic_batch(4, rank=i, image_shape=(2, 16, 128)) for i in range(6)]
            out = {}
            for mode in ("serial", "overlapped", "refused"):
                model = _dp_trainer(level, batches, keep=keep)
                model.overlap_reduce = mode != "serial"
                if mode == "refused":
                    def refuse(params):
                        raise RuntimeError("simulated failure of a collective under stream capture")
                    model._reduce_in_capture = refuse
                for step in range(4):
                    d_loss, g_loss = model.train_step()
                assert model._comm is not None
                if mode == "overlapped":
                    P = model._pipe
                    assert P is not None and P["d"]["reduces"] and P["g"]["reduces"] and model._g_pending is not None
                elif mode == "refused":
                    assert not model._graph_allreduce and not model._pipelined_ok()
                else:
                    assert model._pipe is None
                model.synchronize()   # (applies the generator's pending update)
                assert model._g_pending is None
                out[mode] = (float(d_loss), float(g_loss), model.d_params.flat.clone(), model.g_params.flat.clone(), model.global_step)
            for mode in ("overlapped", "refused"):
                assert out[mode][4] == out["serial"][4] == 4
                _same_up_to_accumulation_order(out["serial"][0], out[mode][0], f"{mode} level {level}: D loss")
                _same_up_to_accumulation_order(out["serial"][1], out[mode][1], f"{mode} level {level}: G loss")
                _same_up_to_accumulation_order(out["serial"][2], out[mode][2], f"{mode} level {level}: discriminator parameters")
                _same_up_to_accumulation_order(out["serial"][3], out[mode][3], f"{mode} level {level}: generator parameters")
        # (iii) where the collective sits, as time: configs[1] itself (full size, bf16, batch 8), where part A of the discriminator run
        # (the real batch's trunk) and of the generator run (forward + mode-seeking first-order pass) are each well over 300 us of kernels
        batches = [R.synthetic_batch(8, rank=i, image_shape=(2, 128, 1024)) for i in range(3)]
        ms = {}
        for mode in ("serial", "one graph", "overlapped"):
            for marker in (0, 300):
                os.environ["GS_COMM_MARKER_US"] = str(marker)
                model = _dp_trainer(1.0, batches, full=True, dtype=torch.bfloat16, keep=False)
                model.overlap_reduce = mode == "overlapped"
                model.fuse_iteration = mode == "one graph"   # (round 6: the iteration as ONE graph, the generator's all-reduce at the front of the NEXT
                                                             #  iteration's fake pass, issued first -- part of it disappears behind the real pass)
                for _ in range(3):
                    model.train_step()
                model.synchronize()
                best = 1e9
                for _ in range(4):
                    t0 = time.perf_counter()
                    for _ in range(5):
                        model.train_step()
                    model.synchronize()
                    best = min(best, (time.perf_counter() - t0) / 5 * 1e3)
                ms[(mode, marker)] = best
                del model
        print("ms per iteration (mode, marker us):", {k: round(v, 3) for k, v in ms.items()})
        serial = ms[("serial", 300)] - ms[("serial", 0)]
        assert serial > 0.45                                            # two 300 us stand-ins on the critical path
        assert ms[("overlapped", 300)] - ms[("overlapped", 0)] < 0.3   # beside part A: neither shows (0.01-0.2 measured, box to box)
        # the one-graph iteration keeps its compute branches (the overlapped form has none: four branchy graphs per iteration would be host-bound);
        # how much of its two collectives the runtime lets run beside compute is reported, not asserted (profiles/r06_g_dp_markers.txt: 0.37-0.61 ms
        # of the 0.6 ms, depending on which chains of the graph end up sharing a hardware queue)
        assert ms[("one graph", 0)] < ms[("overlapped", 0)] - 0.2
        assert ms[("one graph", 300)] - ms[("one graph", 0)] < serial + 0.2
    finally:
        os.environ.pop("GS_COMM_MARKER_US", None)
        dist.destroy_process_group()


def test_full_size_progressive_schedule_end_to_end():
    """BASELINE.json configs[4] at FULL size on the one GPU there is: the whole progressive schedule 2x16 -> 128x1024 (gan_synth_main.py:51-54,
    networks.py:24-29) with growing_steps shortened to 1000 so that 520 iterations walk through every one of the eight graph regimes
    (the 2x16 stage, six fade-ins, fully grown) -- batch 8, 64000-sample notes through the HIP spectral front end into
    [8, 2, 128, 1024] real images, hipGraphs re-captured at every regime change, the fade weight read from device memory.
    Checks: every regime visited in order, losses finite throughout, parameters finite, every colour block's gradient path used
    at least once (its Adam second moment is non-zero), global_step bookkeeping."""
    from gansynth_amd import variables
    from gansynth_amd.dataset import synthetic_nsynth_input_fn
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict

    growing_steps, total = 1000, 520
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    holder = {}
    pg = PGGAN(min_resolution=[2, 16], max_resolution=[128, 1024], min_channels=32, max_channels=256,
               growing_level=lambda: holder["m"].global_step / growing_steps)
    notes = synthetic_nsynth_input_fn(8, range(24, 85), device="cuda", seed=3, num_batches=6)
    pool = [notes() for _ in range(6)]          # six batches of generated notes, cycled (the generator itself is tests/test_dataset*)
    cursor = [0]

    def real_input_fn():
        cursor[0] += 1
        return pool[cursor[0] % len(pool)]

    gen = torch.Generator(device="cuda").manual_seed(5)
    spectral = Dict(waveform_length=64000, sample_rate=16000, spectrogram_shape=[128, 1024], overlap=0.75)
    model = GANSynth(pg.generator, pg.discriminator, real_input_fn, lambda: torch.randn(8, 256, device="cuda", generator=gen), spectral,
                     Dict(R.DEFAULT_HYPER), dtype=torch.bfloat16, use_graphs=True)
    holder["m"] = model
    regimes, losses = [], []
    orig = model.train_step

    def step():
        head, fade = pg._head_depth(pg.growing_depth)
        if not regimes or regimes[-1] != (head, fade is not None):
            regimes.append((head, fade is not None))
        out = orig()
        if model.global_step % 20 == 0:
            losses.append((float(out[0]), float(out[1])))
        return out

    model.train_step = step
    model.train(total_steps=total, log=None)
    assert model.global_step == total and model.d_params.t == total and model.g_params.t == total
    assert regimes == [(0, False)] + [(d, True) for d in range(1, 7)] + [(6, False)], regimes
    assert all(np.isfinite(a) and np.isfinite(b) for a, b in losses), losses
    assert torch.isfinite(model.g_params.flat).all() and torch.isfinite(model.d_params.flat).all()
    for params in (model.g_params, model.d_params):
        for name, p in params.named.items():
            if "color_block" in name:
                off = (p.data.data_ptr() - params.flat.data_ptr()) // 4
                assert float(params.v[off:off + p.numel()].abs().max()) > 0, name   # every head was trained at some depth
    assert replaying_graphs(model, (6, True))
