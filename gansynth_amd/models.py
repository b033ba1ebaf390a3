"""GANSynth trainer step on the HIP path (reference models.py:8-108, train loop :189-194).

Same constructor as the reference's GANSynth (generator / discriminator callables, input fns,
spectral_params, hyper_params).  One iteration = a discriminator update then a generator update,
each on its own fresh batch, exactly like the two session.run calls of models.py:191-192:

  D run: L_D = mean(softplus(-r) + softplus(f) + w_r1 * sum((d sum(r) / d x_real)^2))   :39-49,65
  G run: L_G = mean(softplus(-f) + w_ms / (sum((d sum(G(z)) / d z)^2) + 1e-6))            :57-64
  both with tf.train.AdamOptimizer (TF form), only the G run bumps global_step            :67-89

Parameters, gradients and Adam slots of each network live in one flat fp32 buffer (one fused
Adam launch, one all-reduce payload).  Data parallelism (new -- the reference is single GPU):
one process per GPU, gradients summed with torch.distributed all_reduce (backend "nccl" = RCCL
over xGMI) and averaged inside the Adam kernel.

This module keeps the reference's surface (GANSynth, PitchClassifier) and is the import path for everything outside the package.  GANSynth's
mix-ins hold the rest: iteration.py (the three iteration forms under hipGraph replay), capture.py (how a run is captured and replayed),
data_parallel.py (all-reduce, agreement between ranks); flat_params.py is the flat parameter buffer, fork_probe.py the check of the runtime.
"""
import contextlib
import math
import os

import torch
import torch.nn.functional as TF

from . import config
from . import functional as F
from . import kernels
from . import spectral_ops
from . import variables
from .capture import Capture
from .data_parallel import DataParallel
from .flat_params import _FlatParams
from .fork_probe import _hw_queues_allow_branches
from .iteration import Iterations

_DEFER_REDUCTIONS = not config.flag("GS_NO_DEFERRED_REDUCE")   # A/B switches for measurements
_FUSED_LOSSES = not config.flag("GS_NO_FUSED_LOSSES")
_BATCH_D_TAIL = not config.flag("GS_NO_D_TAIL_BATCH")   # A/B switch: real + fake through the discriminator's tail as one batch
# The all-reduce beside part A of the other run (forked graph branch, four graphs per iteration) is opt-in: the two-graph form with the collective as the LAST node of each run's graph keeps the compute branches of section 6.5 (a four-graph
# iteration with branches would be launch-bound) -- 5.16 against 5.68 ms at world size 1, i.e. the overlapped form has to hide more than
# half a millisecond of all-reduce to break even.
_OVERLAP_REDUCE = config.flag("GS_OVERLAP_REDUCE") and not config.flag("GS_NO_OVERLAP_REDUCE")
_GRAPH_ALLREDUCE = not config.flag("GS_NO_GRAPH_ALLREDUCE")   # A/B switch: the gradient all-reduce as a node of the captured graph
_FORK = not config.flag("GS_NO_FORK")   # A/B switch: independent sub-passes of a run on a forked branch of its hipGraph (GANSynth._branch)
EARLY_FLUSH_DIVS = [int(d) for d in config.value("GS_EARLY_FLUSH_DIV", "16").split(",")]   # a layer is "large" from 1/DIV of the full resolution's pixels (several: one early contraction each)
EARLY_FLUSH_CUS = int(config.value("GS_EARLY_FLUSH_CUS", "192"))   # see GANSynth._early_flush
_FORK_EAGER = config.flag("GS_FORK_EAGER")   # tests: the same branches with eager launches (a second stream, event hops)
_EMA_BEFORE_REFRESH = config.flag("GS_EMA_BEFORE_REFRESH")   # A/B switch: see Iterations._apply_in_graph
AVERAGE_SUFFIX = "/ExponentialMovingAverage"   # tf.train.ExponentialMovingAverage's shadow variable of <variable>


class GANSynth(Iterations, DataParallel, Capture):

    def __init__(self, generator, discriminator, real_input_fn, fake_input_fn, spectral_params, hyper_params,
                 dtype=torch.float32, store=None, distributed=False, use_graphs=False, bucket_bytes=None, keep_gradients=False):
        self.generator, self.discriminator = generator, discriminator
        self.real_input_fn, self.fake_input_fn = real_input_fn, fake_input_fn
        self.spectral_params, self.hyper_params = spectral_params, hyper_params
        self.dtype = dtype
        self.store = store if store is not None else variables.default_store()
        self.distributed = bool(distributed)
        self.world = torch.distributed.get_world_size() if self.distributed else 1
        self.rank = torch.distributed.get_rank() if self.distributed else 0
        self.bucket_bytes = None if bucket_bytes is None else int(bucket_bytes)   # gradient all-reduce granularity (None: see _build)
        # False: the optimizer step clears the flat gradient it consumed (one pass less per run: the next run accumulates from zero);
        # True: `p.grad` of every variable still holds the run's (all-reduced, unscaled) gradient after the step -- tests, inspection
        self.keep_gradients = bool(keep_gradients)
        self._inflight = None                   # (params, [(bucket, work)]) all-reduces launched during the eager backward's tail
        self._comm = None                       # comm.RcclComm: the gradient all-reduce on the backward's own stream (HIP + nccl only)
        self._peeked = None                     # a batch fetched ahead of the first step (train: eager build / restore)
        self._keep_waveforms = False            # train() with summaries on: _real_batch keeps the waveforms of the batch it converted
        self._real_waveforms = None
        self._run_reduced = False               # the last _run replayed a graph that contains its own gradient all-reduce
        self._captured_reduce = False
        self._graph_allreduce = _GRAPH_ALLREDUCE   # cleared for the life of the model if a capture with the collective inside fails
        self.global_step = 0
        self.g_params = None
        self.d_params = None
        self.generator_loss = None
        self.discriminator_loss = None
        # hipGraph replay of the iteration (launch-bound otherwise: ~600 kernels per run); which form runs when: iteration.py
        self.use_graphs = bool(use_graphs)
        self._graphs = {}
        self.restored_from = None
        self._graph_key, self._lerp = None, None
        self.overlap_reduce = _OVERLAP_REDUCE   # data parallel, opt-in: the pipelined iteration (iteration.py)
        self._pipe = None         # the pipelined iteration's two captured pairs and their key
        self._pipe_capture = False
        self._warming_up = False
        # Forked branches inside a run's hipGraph (see _branch): a run is a chain of ~370 kernels of which ~150 are few-block launches of
        # the <= 8x64 levels -- 200 CUs idle while they run -- and it holds sub-passes that do not depend on each other.
        # (data parallel: off in the PIPELINED iteration -- a graph with parallel branches costs the host 1.8 ms per replay instead of 0.06
        #  (scripts/replay_host_time.py), and that iteration replays FOUR graphs: it would be launch-bound; decided in _build, when the
        #  transport is known.  The two-graph data-parallel forms keep their branches.)
        self.fork = _FORK and _hw_queues_allow_branches()
        self.fork_eager = _FORK_EAGER
        self.fork_marks = not config.flag("GS_NO_FORK_MARKS")   # (debugging: branches start where they are opened)
        self._side = None
        self._side2 = None        # the stream of the generator run's own-network nodes beside the discriminator run (_capture_merged)
        self.bucket_d_reduce = config.flag("GS_DP_BUCKET_D")   # (data parallel, captured discriminator run, opt-in: _arm_first_bucket)
        self.first_bucket = None  # (the range of the flat gradient the first message of the last captured discriminator run covers)
        self._split_at = None     # (see _arm_first_bucket)
        self._first_bucket_stream = None
        self._side3 = None
        self._nodes_on_side2 = False
        self._origin = None
        self._after_loss = None
        self.merge_runs = not config.flag("GS_NO_MERGED_RUNS")   # A/B switch: see _train_step_merged
        self._merged = None
        # The WHOLE iteration as one hipGraph with both optimizer steps inside (see "one graph per iteration" above _capture_merged)
        self.fuse_iteration = not config.flag("GS_NO_FUSED_ITERATION")
        self._opt_scalars = None      # functional.DeviceScalars: [lr_t of the discriminator's step, lr_t of the generator's PENDING step | < 0]
        self._before_fake = None      # hook: issued on the fake pass's stream right before the generator's forward of a discriminator run
        self.split_g_loss = not config.flag("GS_NO_SPLIT_G_LOSS")   # A/B switch, see _g_losses_b
        self.split_final_flush = not config.flag("GS_NO_SPLIT_FINAL_FLUSH")   # A/B switch, see kernels.HipKernels._flush_groups
        self._g_pending = None        # lr_t of a generator step whose gradient is in the flat buffer and whose update has not run yet
        # The averaged generator (progressive GAN's recipe; DESIGN.md "Averaged generator"): an exponential moving average of the generator's
        # weights, updated behind every one of its Adam steps.  0 = off: no buffer, no launch, no checkpoint key.
        self.average_decay = self._checked_decay(hyper_params.get("generator_average_decay"))
        self.ema_before_refresh = _EMA_BEFORE_REFRESH
        self._g_pending_om = None     # 1 - decay_t of that pending step (averaging on)
        self._average_in = False      # inside averaged_generator(): g_params.flat holds the AVERAGE, g_params.avg the live weights
        self._marks = {}
        self._serial_run = False
        self._branched = False
        self.branches_opened = 0   # (tests / bench: how many branches the last captures opened)
        self.early_flush = not config.flag("GS_NO_EARLY_FLUSH")   # A/B switch: see _early_flush
        self.batch_d_tail = None   # None: the discriminator's tail over [real; fake] as one batch unless the runs fork (see _batched_tail)
        self.early_flush_always = False   # (tests: the same flush points without branches -- in place, on the one stream)
        self.early_flushes = 0

    # ---------------------------------------------------------------------- averaged generator
    @staticmethod
    def _checked_decay(decay):
        if decay is None:
            return 0.0
        decay = float(decay)
        if not 0.0 <= decay < 1.0:   # (NaN fails both comparisons)
            raise ValueError(f"hyper_params.generator_average_decay must lie in [0, 1) (0 or None: no averaged generator), got {decay!r}")
        return decay

    def _averaging(self):
        return self.average_decay > 0.0

    def _one_minus(self, t):
        """1 - decay_t of the average's update behind the generator's t-th Adam step, decay_t = min(decay, (1 + t) / (10 + t)): the
        `num_updates` warm-up of tf.train.ExponentialMovingAverage (without it the average at step 100 is still 90 % initialisation noise
        at decay 0.999).  Computed in float64 and rounded to fp32 ONCE: the value the kernel multiplies by."""
        decay_t = min(self.average_decay, (1.0 + t) / (10.0 + t))
        return float(torch.tensor(1.0 - decay_t, dtype=torch.float64).to(torch.float32))

    def _average_after(self, params):
        """Behind an Adam step of `params` (params.t counts it): the average follows the generator's; the discriminator has none.
        Data parallel: the average is a function of the weights alone, which are identical on every rank after the all-reduced step --
        so is the average, with no communication."""
        if params is not self.g_params or not self._averaging():
            return
        K = kernels.get()
        one_minus = self._one_minus(params.t)
        if hasattr(K, "ema_step"):
            K.ema_step(params.avg, params.flat, one_minus)
        else:   # (a backend without the kernel -- the tests' CPU emulation: the same rule in torch, fp32)
            params.avg.sub_((params.avg - params.flat) * one_minus)

    def _swap_average(self):
        """g_params.flat <-> g_params.avg in place (every pointer a captured graph or a variable view holds stays valid, and there is no
        third buffer), then the generator's prepared operands are rebuilt from what `flat` holds now."""
        K = kernels.get()
        g = self.g_params
        if hasattr(K, "swap_"):
            K.swap_(g.flat, g.avg)
        else:
            with torch.no_grad():
                live = g.flat.clone()
                g.flat.copy_(g.avg)
                g.avg.copy_(live)
        if hasattr(K, "invalidate_weights"):
            K.invalidate_weights(g.flat)
            K.refresh_weights(g.flat)

    @contextlib.contextmanager
    def averaged_generator(self):
        """`with model.averaged_generator():` -- inside, the generator runs on its AVERAGED weights: the pending update is joined, the live
        weights and the average change places (_swap_average), and they change back on the way out, also when the body raises.  Inside,
        train_step / discriminator_step / generator_step / state_dict / checkpoint.save / load raise RuntimeError.  Data parallel: entering
        joins the pending update as the other readers do -- a collective when `collective_pending()`, so every rank enters together."""
        if self.g_params is None or self.g_params.avg is None:
            first = "generator/..." if self.g_params is None else next(iter(self.g_params.named))
            raise ValueError(f"the model keeps no averaged generator ({first}{AVERAGE_SUFFIX} and the rest): build it with "
                             f"hyper_params.generator_average_decay, or restore a checkpoint that holds the averages (weights='average' "
                             f"with a model_dir)")
        self._refuse_while_averaged("averaged_generator (it does not nest)")
        self._join_updates()
        self._swap_average()
        self._average_in = True
        try:
            yield self
        finally:
            self._average_in = False
            self._swap_average()

    def _refuse_while_averaged(self, what):
        if self._average_in:
            raise RuntimeError(f"{what}: the generator's average is swapped in (inside averaged_generator()); leave the context first")

    def _restore_for(self, model_dir, weights):
        """The restore of generate / evaluate / synthesize, BEFORE any swap.  weights="average" on a model built without a decay takes the
        average from the checkpoint (and allocates its buffer): no model_dir, no checkpoint there, or a file without the averages is a
        ValueError naming the first missing key -- never the live weights under another name."""
        from . import checkpoint
        if weights not in ("live", "average"):
            raise ValueError(f"weights must be 'live' or 'average' (got {weights!r})")
        need = weights == "average" and self.g_params.avg is None
        if model_dir is None:
            restored = None
        else:
            restored = checkpoint.restore(self, model_dir, require_average=need)
        if need and restored is None:
            first = next(iter(self.g_params.named)) + AVERAGE_SUFFIX
            where = "no model_dir was given" if model_dir is None else f"{model_dir} holds no checkpoint"
            raise ValueError(f"weights='average': the model was built without generator_average_decay and {where} to take {first} from")
        return restored

    # ------------------------------------------------------------------------ forked branches
    # A run holds sub-passes that do not depend on each other:
    #   G run: D(G(z)) forward                        ||  the mode-seeking first-order pass d sum(G(z)) / dz     (both need G(z) only)
    #          backward through D down to d L / d G(z) ||  the second-order pass of the mode-seeking term        (both need the loss head only)
    #   D run: G(z) forward (no grad)                  ||  D's trunk on the real batch
    # Each side has its own latency-bound stretch (the <= 8x64 levels: 64-block launches of ~10 us on a 256-CU chip) that the other side's
    # full-chip convs can fill.  Inside a stream capture a second stream is free -- fork and join become edges of the hipGraph, there is no
    # event hop at replay -- so the second member of each pair runs on a side stream THERE (and only there: between eager launches an event
    # hop costs more than the overlap gains).  autograd runs a node's backward on the stream its forward ran on and orders the streams with
    # events (captured as edges too), so putting D's forward on the side stream is what puts D's backward beside the second-order pass.
    # The host-side launch ORDER is the same with and without branches (the engine's ready queue does not look at streams): the same kernels
    # on the same operands, hence bit-identical parameters -- tests/test_model_gpu.py::test_forked_branches_change_nothing_but_the_schedule.
    # Memory: torch's caching allocator hands a freed block back to the stream that allocated it, so a tensor read on the other stream must
    # not be recycled under that read: kernels.HipKernels.stream_guard() marks every tensor argument of every kernel-layer call with the
    # stream it is used on (record_stream; inside a capture such a block is simply not reused before the capture ends).
    def _forking(self):
        if not self.fork or not torch.cuda.is_available() or not hasattr(kernels.get(), "stream_guard"):
            return False
        return self._capturing() or (self.fork_eager and not self._warming_up)

    def _fork_mark(self, tag):
        """Remember this point of the current stream: a branch opened later IN THE SAME capture starts from here, not from the stream's end
        (serial runs only: the two parts of a pipelined run are two graphs, and an event of one capture cannot be waited on in another)."""
        self._marks.pop(tag, None)
        if self._serial_run and self._forking() and self.fork_marks:
            ev = torch.cuda.Event()
            ev.record()
            self._marks[tag] = ev

    @contextlib.contextmanager
    def _branch(self, tag=None, join=True):
        """`with self._branch(tag):` -- the launches inside go on the side stream, which starts at the mark `tag` (or here) and which the
        current stream waits for at the end of the block.  A no-op outside a capture."""
        ev = self._marks.pop(tag, None) if tag is not None else None
        if not self._forking():
            yield
            return
        main = torch.cuda.current_stream()
        self._second_stream("_side", [main, self._side2])
        side = self._side
        if ev is not None:
            side.wait_event(ev)
        else:
            side.wait_stream(main)
        self.branches_opened += 1
        self._branched = True
        with torch.cuda.stream(side):
            yield
        if join:   # (else: at the end of the run, _part_b)
            main.wait_stream(side)

    def _early_flush(self, select, then=None):
        """kernels.HipKernels.early_flush_rule: the weight gradients of the full-chip levels recorded so far are contracted NOW -- on the
        branch when the run is being captured (joined at the end of the run), else in place: the same launches on the same operands either
        way.  (Called from inside a backward node, i.e. on autograd's device thread, under that node's stream.)"""
        K = kernels.get()
        self.early_flushes += 1
        was = K.lib.gs_wgrad_cu_cap(EARLY_FLUSH_CUS) if hasattr(K, "lib") else 0   # (the chain beside it needs somewhere to land)
        cur = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else None
        on_branch = self._side is not None and cur == self._side.cuda_stream
        # A node of the merged iteration's generator part runs on ITS stream: the contraction then goes to the run's own stream (idle while the
        # backward walks that one), never to the other branch -- two non-origin streams of a capture that wait on each other's events become each
        # other's parent in hip::Stream's bookkeeping and hip::Stream::EndCapture recurses until the stack runs out (ROCm 7.0.2).
        on_side2 = self._side2 is not None and cur == self._side2.cuda_stream and self._origin is not None and self._forking()
        try:
            if on_side2:
                self._origin.wait_stream(self._side2)
                with torch.cuda.stream(self._origin):
                    K.flush_wgrad_reductions(select=select)
                    if then is not None:
                        then()
                return
            with (contextlib.nullcontext() if on_branch else self._branch(join=False)):   # (a node of the branch itself: in place)
                K.flush_wgrad_reductions(select=select)
                if then is not None:
                    then()
        finally:
            if hasattr(K, "lib"):
                K.lib.gs_wgrad_cu_cap(was)

    def _large_layer_pixels(self):
        owner = getattr(self.generator, "__self__", None)
        if owner is None or not hasattr(owner, "resolution"):
            return None
        full = int(owner.resolution(owner.max_depth).prod())
        return [max(1, full // d) for d in EARLY_FLUSH_DIVS]   # (16: the three levels at the top of the pyramid)

    # ----------------------------------------------------------------------------- build
    def _build(self, latents, labels):
        """Create every variable (the reference's graph owns all of them from step 0), then flatten."""
        owner = getattr(self.generator, "__self__", None)
        with torch.no_grad():
            if owner is not None and hasattr(owner, "_g_variables"):
                with variables.variable_scope("generator"):
                    owner._g_variables(latents.shape[1], labels.shape[1])
                with variables.variable_scope("discriminator"):
                    owner._d_variables(labels.shape[1])
            else:
                images = self.generator(latents, labels)
                self.discriminator(images, labels)
        self.g_params = _FlatParams(self.store.trainable_variables("generator"))
        self.d_params = _FlatParams(self.store.trainable_variables("discriminator"))
        if self.distributed:  # identical weights on every rank
            from . import comm
            if self._comm is None and not config.flag("GS_TORCH_COLLECTIVES"):
                self._comm = comm.create(self.g_params.flat.device)   # RCCL on the backward's own stream (None on CPU / gloo)
            if self._comm is not None:
                self._comm.broadcast_(self.g_params.flat, 0)
                self._comm.broadcast_(self.d_params.flat, 0)
            else:
                torch.distributed.broadcast(self.g_params.flat, 0)
                torch.distributed.broadcast(self.d_params.flat, 0)
            if self.bucket_bytes is None:
                # same-stream RCCL: collectives and updates are serial on the one stream whatever the granularity, so ONE
                # all-reduce per network (fewest launches); torch.distributed's own collectives run on the communicator's stream
                # and do overlap the per-bucket updates: 8 MiB buckets there
                self.bucket_bytes = (64 << 20) if self._comm is not None else (8 << 20)
            self.g_params.make_buckets(self.bucket_bytes // 4, reverse=True)
            self.d_params.make_buckets(self.bucket_bytes // 4, reverse=False)
            if self._overlap_in_graph() or self._comm is None:
                # the pipelined four-graph iteration (see __init__); and torch.distributed's collectives, which run on THEIR stream beside the
                # launches that follow them: with the passes apart and the early contraction the world-1 step was no longer bit-identical to
                # the non-distributed one there (5e-7 on the parameters, cause not found) -- that transport keeps round 4's schedule
                self.fork = False
        if self._averaging():
            # from the initial weights (behind the broadcast: the same on every rank, and it stays the same with no communication --
            # the average is a function of the weights, _average_after)
            self.g_params.enable_average()
        K = kernels.get()
        if hasattr(K, "register_param_buffer"):  # lets the conv kernels keep their re-laid weight operands between calls
            K.register_param_buffer(self.g_params.flat)
            K.register_param_buffer(self.d_params.flat)
            K.invalidate_weights()

    def _ensure_built(self, latents, labels):
        if self.g_params is None:
            self._build(latents, labels)

    # -------------------------------------------------------------------------- inputs
    def _real_batch(self):
        """real_input_fn() -> (waveforms [B,L] | images [B,2,T,F], labels [B,61])."""
        data, labels = self.real_input_fn()
        if data.dim() == 2:  # waveforms: models.py:27-28
            images = spectral_ops.convert_to_images(data, **self.spectral_params, dtype=self.dtype)
        else:
            images = data
        if self._keep_waveforms:   # (the audio summary of the real side: models.py:141)
            self._real_waveforms = data if data.dim() == 2 else None
        return images.to(self.dtype), labels.to(self.dtype)

    # --------------------------------------------------------------------------- losses
    @staticmethod
    def _label_logits(logits, labels):
        """tf.gather_nd(logits, tf.where(labels)) for one-hot labels (models.py:39-40)."""
        # (labels are one-hot: the product is exact in the activation dtype and the fp32 sum has one non-zero term)
        return (logits * labels.to(logits.dtype)).sum(dim=1, dtype=torch.float32)

    # Each run splits into a part that touches only the network being updated and a part that needs the other network:
    #   D run:  A = D(real) + the R1 first-order pass          B = G(z) (no grad), D(fake), loss, backward
    #   G run:  A = G(z) + the mode-seeking first-order pass    B = D(G(z)), loss, backward
    # (`_a` functions return what `_b` needs).  The pipelined step overlaps the gradient all-reduce of one network (a forked
    # branch of the part-A graph) with part A of the other network's run.
    # `fused`: the loss algebra on the [N] / [N, C] tensors -- label-logit select, softplus, penalty, mean, and their autograd
    # mirror images, ~50 torch launches per iteration -- as ONE kernel per loss (gs_gan_d_loss / gs_gan_g_loss: value and
    # gradients); `_b` then returns the mean loss itself instead of the per-sample losses.  The public *_losses methods keep
    # the per-sample form of the reference.
    def _fused_losses(self):
        # (the one-launch discriminator loss carries ONE penalty term: with the optional penalty on the generator distribution,
        # models.py:50-54 -- weight 0 in the shipped configuration -- the per-sample algebra runs instead)
        return _FUSED_LOSSES and hasattr(kernels.get(), "gan_d_loss") and not self.hyper_params.get("fake_gradient_penalty_weight", 0.0)

    def _batched_tail(self, fused, images):
        """The discriminator run sends the real and the fake batch through the latency-bound tail of the network (8x64 and below: a few
        tens of blocks per launch on 256 CUs) as ONE batch of 2n -- half the launches there, forward and backward; the R1 pass seeds the
        real rows only.  Needs the network in two pieces (networks.PGGAN.discriminator_trunk / _tail) and the one-launch loss.  (An
        activation tap still sees two passes: functional.tap_pair.)"""
        owner = getattr(self.discriminator, "__self__", None)
        # With forked branches the two passes stay apart instead: the whole fake pass (G(z), D's trunk AND tail, and through autograd their
        # backward) runs on the branch beside the real pass with its R1 passes -- twice the few-block launches of the tail, on two streams
        # that fill each other's gaps: 5.74 -> 5.42 ms against the batched tail (same box).  `batch_d_tail` overrides (tests).
        want = self.batch_d_tail if self.batch_d_tail is not None else (_BATCH_D_TAIL and not self.fork)
        return (want and fused and images.is_cuda and hasattr(owner, "discriminator_trunk")
                and getattr(self.discriminator, "__func__", None) is getattr(type(owner), "discriminator", None)
                and hasattr(kernels.get(), "lib"))

    def _d_losses_a(self, labels, real_images, fused=False):
        hp = self.hyper_params
        self._fork_mark("d_root")   # (the generator's no-grad forward of part B needs nothing of this part: it branches off here)
        real_images = real_images.detach().requires_grad_(True)
        if self._batched_tail(fused, real_images):   # part A is the real batch's trunk; everything else needs the fake batch beside it
            owner = self.discriminator.__self__
            return ("trunk", real_images) + tuple(owner.discriminator_trunk(real_images, labels.shape[1])) + (F.tap_index(),)
        _, raw = self.discriminator(real_images, labels)
        real_logits = None if fused else self._label_logits(raw, labels)
        penalty = None
        if hp.real_gradient_penalty_weight:
            with F.data_grads_only():   # tf.gradients(real_logits, [real_images]) (models.py:47): no parameter gradients on this pass
                if fused:   # d sum_i real_logit_i / d logits = the one-hot labels themselves
                    (real_gradients,) = torch.autograd.grad(raw, real_images, grad_outputs=labels.to(raw.dtype), create_graph=True)
                else:
                    (real_gradients,) = torch.autograd.grad(real_logits.sum(), real_images, create_graph=True)
            penalty = F.sumsq_rows(real_gradients)
            if not fused:   # (the fused loss kernel takes the weight itself: no scaling launch, forward or backward)
                penalty = penalty * hp.real_gradient_penalty_weight
        return (raw, penalty) if fused else (TF.softplus(-real_logits), penalty)

    def _d_losses_b(self, part_a, latents, labels, fused=False):
        hp = self.hyper_params
        if isinstance(part_a[0], str):   # ("trunk", ...): the batched-tail form of part A
            return self._d_losses_b_batched(part_a, latents, labels)
        real_part, penalty = part_a
        fake_weight = hp.get("fake_gradient_penalty_weight", 0.0)
        with self._branch("d_root"):   # the whole fake pass beside the real one (its backward then runs on the branch as well)
            self._run_before_fake()
            with torch.no_grad():  # var_list is the discriminator's only: no generator backward (models.py:86-89)
                fake_images = self.generator(latents, labels)
            if fake_weight:   # tf.gradients(fake_logits, [fake_images]) (models.py:51): the images are the point of differentiation
                fake_images = fake_images.detach().requires_grad_(True)
            _, fake_logits = self.discriminator(fake_images, labels)
        if fused:
            return F.gan_d_loss(real_part, fake_logits, labels, penalty, hp.real_gradient_penalty_weight or 1.0)
        fake_logits = self._label_logits(fake_logits, labels)
        losses = real_part + TF.softplus(fake_logits)
        if penalty is not None:
            losses = losses + penalty
        if fake_weight:   # zero-centred gradient penalty on the generator distribution (models.py:50-54): the R1 kernels on the fake batch
            with F.data_grads_only():
                (fake_gradients,) = torch.autograd.grad(fake_logits.sum(), fake_images, create_graph=True)
            losses = losses + F.sumsq_rows(fake_gradients) * fake_weight
        return losses

    def _d_losses_b_batched(self, part_a, latents, labels):
        """models.py:39-54,65 with the two discriminator passes sharing their tail: logits of [real; fake] from one pass, the R1 term
        (models.py:46-49) as the gradient of the real rows' label logits -- the cotangent of the fake rows is zero --, the loss and both
        logit gradients from the one-launch kernel."""
        hp = self.hyper_params
        _, real_images, x_real, depth, fresh, real_call = part_a
        owner = self.discriminator.__self__
        with self._branch("d_root"), torch.no_grad():  # var_list is the discriminator's only: no generator backward (models.py:86-89); beside part A
            self._run_before_fake()
            fake_images = self.generator(latents, labels)
        x_fake, depth_f, fresh_f = owner.discriminator_trunk(fake_images, labels.shape[1])
        assert depth_f == depth and fresh_f == fresh
        with F.tap_pair(real_call, F.tap_index()):
            _, raw = owner.discriminator_tail(F.cat_batch(x_real, x_fake), depth, fresh, labels, sub_batches=2)
        penalty = None
        if hp.real_gradient_penalty_weight:
            n = labels.shape[0]
            seed = self._constant_like(raw, 0)   # (rows n..2n stay zero for the life of the buffer)
            seed[:n].copy_(labels)   # d sum_i real_logit_i / d logits: the one-hot labels on the real rows
            with F.data_grads_only():   # tf.gradients(real_logits, [real_images]) (models.py:47): no parameter gradients on this pass
                (real_gradients,) = torch.autograd.grad(raw, real_images, grad_outputs=seed, create_graph=True)
            penalty = F.sumsq_rows(real_gradients)
        return F.gan_d_loss_pair(raw, labels, penalty, hp.real_gradient_penalty_weight or 1.0)

    def _run_before_fake(self):
        hook, self._before_fake = self._before_fake, None
        if hook is not None:   # (one graph per iteration: the generator's pending update runs HERE, on the fake pass's stream, see _capture_merged)
            hook()

    def discriminator_losses(self, latents, labels, real_images):
        return self._d_losses_b(self._d_losses_a(labels, real_images), latents, labels)

    def _g_losses_a(self, latents, labels, fused=False):
        hp = self.hyper_params
        latents = latents.detach().requires_grad_(True)
        fake_images = self.generator(latents, labels)
        self._fork_mark("g_images")   # (the discriminator's pass over these images in part B does not wait for the first-order pass below)
        mode_seeking = None
        if hp.mode_seeking_loss_weight:
            ones = self._constant_like(fake_images, 1)  # tf.gradients(ys) sums ys
            with F.data_grads_only():   # tf.gradients(fake_images, [latents]) (models.py:60)
                (latent_gradients,) = torch.autograd.grad(fake_images, latents, grad_outputs=ones, create_graph=True)
            if fused:
                mode_seeking = F.sumsq_rows(latent_gradients)   # (the kernel forms weight / (. + 1e-6))
            else:
                mode_seeking = 1.0 / (latent_gradients.float().pow(2).sum(dim=1) + 1.0e-6)
        return fake_images, mode_seeking

    def _g_losses_b(self, part_a, labels, fused=False):
        hp = self.hyper_params
        fake_images, mode_seeking = part_a
        if fused and mode_seeking is not None and self.split_g_loss and self._serial_run_or_merged() and hasattr(F, "gan_g_loss_mode_seeking"):
            # L_G = mean(softplus(-f)) + mean(w / (s + eps)) as TWO roots of one backward call: the mode-seeking half needs nothing of the
            # discriminator, so its second-order pass -- the longest chain of this run -- starts at the run's FIRST node, beside the
            # discriminator's forward over G(z), instead of behind a loss launch that waits for that forward (in a replayed graph a node starts
            # when its dependencies are done, whatever the order it was issued in: DESIGN.md 6.6).  One launch per half; the gradients are the
            # same numbers, the loss value is the sum of the two partial means.
            l_ms = F.gan_g_loss_mode_seeking(mode_seeking, hp.mode_seeking_loss_weight, 1.0e-6)
            with self._branch("g_images", join=False):   # (joined at the end of the run, _part_b)
                _, fake_logits = self.discriminator(fake_images, labels)
                l_adv = F.gan_g_loss(fake_logits, labels, None, 0.0, 1.0e-6)
            return (l_adv, l_ms)
        # (the same split of the DISCRIMINATOR's loss -- real half and fake half as two roots of one backward call -- measured 5.15 -> 5.41 ms: the
        #  fake pass then started 0.9 ms into the graph behind a chain it does not depend on, profiles/r06_p_split_losses_ab.txt; not kept)
        with self._branch("g_images") if mode_seeking is not None else contextlib.nullcontext():
            _, fake_logits = self.discriminator(fake_images, labels)   # (its backward then runs on the branch too: beside the second-order pass)
        if fused:
            return F.gan_g_loss(fake_logits, labels, mode_seeking, hp.mode_seeking_loss_weight, 1.0e-6)
        fake_logits = self._label_logits(fake_logits, labels)
        losses = TF.softplus(-fake_logits)
        if mode_seeking is not None:
            losses = losses + mode_seeking * hp.mode_seeking_loss_weight
        return losses

    def _serial_run_or_merged(self):
        return self._serial_run or self._nodes_on_side2 or self._capturing() or not self._forking()

    def generator_losses(self, latents, labels):
        return self._g_losses_b(self._g_losses_a(latents, labels), labels)

    # ------------------------------------------------------------------------- updates
    def _adam(self, params, lr_t, beta1, beta2):
        """One TF-Adam step of the whole flat buffer on its (reduced) gradient."""
        zero = not self.keep_gradients
        kernels.get().adam_tf_step(params.flat, params.grad, params.m, params.v, lr_t, beta1, beta2, 1.0e-8, 1.0 / self.world, zero_grad=zero)
        params.grad_clean = zero
        self._average_after(params)

    def _part_a(self, which, *inputs):
        """Own-network part of a run (see _d_losses_a / _g_losses_a); also arms the run: requires_grad flags, zeroed gradients."""
        if which == "d":
            self.g_params.requires_grad_(False)
            self.d_params.requires_grad_(True)
            self.d_params.begin_run()
            return self._d_losses_a(*inputs, fused=self._fused_losses())        # (labels, real_images)
        self.g_params.requires_grad_(True)
        self.d_params.requires_grad_(False)
        self.g_params.begin_run()
        return self._g_losses_a(*inputs, fused=self._fused_losses())            # (latents, labels)

    def _part_b(self, which, part_a, *inputs):
        """The rest of the run: losses, backward into the flat gradient buffer; returns the (detached) mean loss."""
        fused = self._fused_losses()
        self._branched = False
        self._origin = torch.cuda.current_stream() if torch.cuda.is_available() else None   # (the stream this run is issued -- or captured -- on)
        losses = self._d_losses_b(part_a, *inputs, fused=fused) if which == "d" else self._g_losses_b(part_a, *inputs, fused=fused)   # (latents, labels) | (labels,)
        multi = losses if isinstance(losses, tuple) else None     # several roots of ONE backward call: see _g_losses_b
        loss = None if multi is not None else (losses if losses.dim() == 0 else losses.mean())   # (the fused loss kernels return the mean itself)
        hook, self._after_loss = self._after_loss, None
        if hook is not None:
            # Merged iteration: part A of the other run forks off HERE and is issued here, in front of this run's backward (see _capture_merged).
            # (Measured round 6, profiles/r06_d_hook_after_backward_ab.txt: issued BEHIND the backward from an event recorded here: 5.23 -> 5.29 ms.)
            hook()
        K = kernels.get()
        deferring = _DEFER_REDUCTIONS and hasattr(K, "defer_wgrad_reductions")   # parameter gradients are only read after the whole backward:
        if deferring:                                        # their ~70 slice reductions are folded in one go at the end
            if hasattr(K, "complete_rule"):
                K.defer_wgrad_reductions(tag=which)
            else:
                K.defer_wgrad_reductions()
        params = self.d_params if which == "d" else self.g_params
        overlap = (self.distributed and deferring and len(params.buckets) > 1 and not self._capturing()
                   and not getattr(self, "_warming_up", False))
        if deferring and self.early_flush and hasattr(K, "early_flush_rule") and (self.fork or self.early_flush_always):
            # (eager launches follow the same rule, in place: a captured run and an eager one then associate every sum alike -- also the
            #  data-parallel eager path, whose buckets go on the wire from the flush at the end of the pass, behind every early launch)
            big = self._large_layer_pixels()
            if big is not None:
                K.early_flush_rule(big, self._early_flush)
        if deferring and which == "d":
            self._arm_first_bucket(K, params)
        launched = []
        if hasattr(F, "reset_fusion_state"):
            F.reset_fusion_state()   # (side-channel state of cross-node fusions is per backward pass)
        def backward(root):
            with (F.params_only() if hasattr(F, "params_only") else contextlib.nullcontext()):   # tf.gradients(loss, var_list): leaf activations want no gradient
                many = list(root) if isinstance(root, (tuple, list)) else None
                first = many[0] if many is not None else root
                if first.is_cuda and first.dim() == 0 and first.dtype == torch.float32 and not self._capturing_fresh_seed(first.device):
                    seed = F.unit_seed(first.device)   # (the loss heads recognise the seed: functional.unit_seed)
                    torch.autograd.backward(many if many is not None else root, grad_tensors=[seed] * len(many) if many is not None else seed)
                elif many is not None:
                    torch.autograd.backward(many)
                else:
                    root.backward()

        try:
            backward(multi if multi is not None else loss)
        finally:
            if hasattr(F, "reset_fusion_state"):
                F.reset_fusion_state()   # (the hand-off table holds tensors of this pass -- of a graph's pool while capturing: not beyond it)
            if deferring:
                if hasattr(K, "early_flush_rule"):
                    K.early_flush_rule(0, None)
                # The final contraction reads the (x, gy) pairs and bias partial rows the branches produced and ADDS into gradients the early
                # contraction on the branch added into (read-modify-write folds, not atomics): it must sit behind the branches in the
                # captured graph, not merely behind them in time.  record_stream keeps the allocator honest and orders nothing; autograd's
                # end-of-backward sync only covers the streams of the leaves it accumulated into.  The join costs nothing: the flush needs
                # those results anyway.  (advisor, round 5)
                self._join_branches()
                if overlap:   # contract the layers bucket by bucket; a finished bucket goes on the wire under the next one's kernels
                    K.flush_wgrad_reductions(group_of=params.bucket_of,
                                             on_group_done=lambda i: launched.append((i, self._launch_reduce(params, i))))
                elif self.split_final_flush and self._forking() and self._side is not None and self._capturing():
                    K.flush_wgrad_reductions(split_stream=self._side)   # (the branch is idle here: joined above)
                else:
                    K.flush_wgrad_reductions()
        if launched:
            self._inflight = (params, launched)
        self._join_branches()   # (a branch opened by the flush itself; a branch left open would fail the capture)
        if multi is not None:
            loss = multi[0].detach()
            for r in multi[1:]:
                if r.is_cuda:
                    r.record_stream(torch.cuda.current_stream())   # (made on its branch's stream, read here)
                loss = loss + r.detach()
        if self.distributed and self._comm is not None and self._graph_allreduce and self._capturing() and not getattr(self, "_pipe_capture", False):
            # Same-stream RCCL is capturable: the all-reduce of this run's flat gradient becomes the LAST NODE of the run's hipGraph, so
            # a replayed run hands over reduced gradients and no eager collective launch sits between the replay and the update.
            split, self._split_at = self._split_at, None
            if self._first_bucket_stream is not None:
                torch.cuda.current_stream().wait_stream(self._first_bucket_stream)
                self._first_bucket_stream = None
            if split:   # (the middle of the buffer went out behind the grouped contractions, _first_bucket_behind_groups: its two ends now)
                for a, b in ((0, split[0]), (split[1], params.grad.numel())):
                    if b > a:
                        self._comm.all_reduce_(params.grad[a:b], marker_share=(b - a) / params.grad.numel())
            else:
                self._reduce_in_capture(params)
            self._captured_reduce = True
        return loss.detach()

    def _join_branches(self):
        """The current stream waits for every branch this run opened: the side stream (every branch was joined where it closed, except the
        early contraction's, and autograd joins the streams it used) and, in the merged iteration, the stream this run's own-network nodes
        ran -- and accumulated -- on."""
        if self._branched:
            self._branched = False
            torch.cuda.current_stream().wait_stream(self._side)
        if self._nodes_on_side2 and self._forking():
            torch.cuda.current_stream().wait_stream(self._side2)

    def _constant_like(self, t, value):
        """A constant tensor of t's shape, layout and dtype, all ones or all zeros, filled once and never written afterwards (of the zeros
        the caller overwrites the same rows every time).  A fill created inside a stream capture would belong to that graph's pool, so
        there the plain fill runs."""
        cache = self.__dict__.setdefault("_constants", {})
        key = (value, tuple(t.shape), tuple(t.stride()), t.dtype, str(t.device))
        c = cache.get(key)
        if c is None:
            c = torch.ones_like(t) if value else torch.zeros_like(t)
            if not self._capturing():
                cache[key] = c
        return c

    def _capturing_fresh_seed(self, device):
        """True when the constant seed of this device would have to be CREATED inside a stream capture (its memory would belong
        to that graph's pool): then the plain loss.backward() runs."""
        if str(torch.device(device)) in F._UNIT:
            return False
        if self._capturing():
            return True
        F.unit_seed(device)
        return False

    def _forward_backward(self, which, *inputs):
        """Gradients of one run into the flat gradient buffer; returns the (detached) mean loss.
        inputs: (latents, labels, real_images) for "d", (latents, labels) for "g"."""
        self._serial_run = True   # (both parts inside one capture: a branch of part B may start at a mark of part A)
        try:
            if which == "d":
                latents, labels, real_images = inputs
                return self._part_b("d", self._part_a("d", labels, real_images), latents, labels)
            latents, labels = inputs
            return self._part_b("g", self._part_a("g", latents, labels), labels)
        finally:
            self._serial_run = False
            self._marks.clear()

    def _regime(self):
        """(head depth, fade weight or None) of the networks at the current growing depth; None for foreign network objects."""
        owner = getattr(self.generator, "__self__", None)
        if owner is None or not hasattr(owner, "_head_depth") or getattr(self.discriminator, "__self__", None) is not owner:
            return None
        return owner._head_depth(owner.growing_depth)

    def discriminator_step(self, latents, labels, real_images):
        self._refuse_while_averaged("discriminator_step")
        self._ensure_built(latents, labels)
        hp = self.hyper_params
        loss = self._run("d", latents, labels, real_images)
        self._apply(self.d_params, hp.discriminator_learning_rate, hp.discriminator_beta1, hp.discriminator_beta2, reduced=self._run_reduced)
        self.discriminator_loss = loss
        return self.discriminator_loss

    def generator_step(self, latents, labels):
        self._refuse_while_averaged("generator_step")
        self._ensure_built(latents, labels)
        hp = self.hyper_params
        loss = self._run("g", latents, labels)
        self._apply(self.g_params, hp.generator_learning_rate, hp.generator_beta1, hp.generator_beta2, reduced=self._run_reduced)
        self.global_step += 1  # models.py:84
        self.generator_loss = loss
        return self.generator_loss

    @staticmethod
    def _lr_t(lr, beta1, beta2, t):
        return lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)

    def _next_inputs(self):
        """One iteration's inputs (models.py:191-192: a fresh batch for each of the two runs).  StopIteration = the input ran dry."""
        if self._peeked is not None:
            out, self._peeked = self._peeked, None
            return out
        real_images, labels = self._real_batch()
        d_latents = self.fake_input_fn().to(self.dtype)
        # the G run only consumes the labels of its batch (waveform branch is pruned): a feed that can advance one batch and hand
        # over its labels alone (bank.BankFeed.next_labels) is asked for just that -- the same batch position either way
        next_labels = getattr(self.real_input_fn, "next_labels", None)
        g_labels = next_labels() if next_labels is not None else self.real_input_fn()[1]
        g_latents, g_labels = self.fake_input_fn().to(self.dtype), g_labels.to(self.dtype)
        return real_images, labels, d_latents, g_latents, g_labels

    def train_step(self):
        """models.py:191-192: one discriminator run then one generator run, fresh inputs for each."""
        self._refuse_while_averaged("train_step")
        real_images, labels, d_latents, g_latents, g_labels = self._next_inputs()
        self._ensure_built(d_latents, labels)
        if self.use_graphs:
            self._check_fork_runtime()
        if self._pipelined_ok():
            return self._train_step_pipelined(d_latents, labels, real_images, g_latents, g_labels)
        if self._merged_ok():
            return self._train_step_merged(d_latents, labels, real_images, g_latents, g_labels)
        return self._plain_iteration(d_latents, labels, real_images, g_latents, g_labels)

    def train(self, model_dir=None, config=None, total_steps=None, save_checkpoint_steps=1000, save_summary_steps=None, log_tensor_steps=100,
              log=print, save=None):
        """models.py:110 -- `train(model_dir, config, total_steps, save_checkpoint_steps, save_summary_steps, log_tensor_steps)`, the
        reference's own signature and argument order, so that gan_synth_main.py:102-109 calls it unchanged.  `config` is the reference's
        tf.ConfigProto (session / GPU-allocator options, gan_synth_main.py:91-98): nothing of it applies to this runtime, it is accepted
        and ignored.  `log`, `save` are additions (keyword only in practice).
        models.py:110-194: resume from the latest checkpoint of `model_dir` (CheckpointSaverHook / MonitoredSession semantics),
        alternate D and G runs until global_step reaches total_steps (StopAtStepHook) or the input runs dry (OutOfRangeError, :193),
        log the two losses every `log_tensor_steps` (LoggingTensorHook), checkpoint every `save_checkpoint_steps` and at the end.
        `save_summary_steps` (honoured when truthy and `model_dir` is given; the default None keeps summaries off): the three
        SummarySaverHooks of models.py:131-174 -- whenever global_step % save_summary_steps == 0 after a step, one Event record each
        for audio (real_waveforms, fake_waveforms), images (real / fake magnitude_spectrograms and instantaneous_frequencies, four
        items each) and scalars (generator_loss, discriminator_loss), in that order, into the events file of `model_dir`
        (summary.SummaryWriter; a record that would hold no value is not written).  The real side is the batch the discriminator run
        just used; real_waveforms only when the input gave waveforms, fake_waveforms only with `spectral_params`.  Two differences from
        the reference: TF's hook also fires on the first run of a session, this one follows the modulus rule of the logs and the
        checkpoints alone; and the reference fetches the fake side inside the training run, while this tree summarises AFTER the update
        -- a no-grad generator pass over that iteration's generator-run latents and labels, eagerly between two replays of the captured
        iteration, drawing no random number and leaving the training trajectory bit for bit as it is without summaries.  The file is
        flushed at every checkpoint and at the end.
        Data parallel: EVERY rank passes `model_dir` and restores from the same file (weights, Adam slots, optimizer steps, global_step
        -- so that all ranks resume in the same growing regime); only rank 0 saves (`save` defaults to rank == 0) and summarises, and
        every rank joins the pending update at a summary step as at a checkpoint."""
        if isinstance(model_dir, (int, float)) and not isinstance(model_dir, bool) and total_steps is None:
            model_dir, total_steps = None, model_dir   # (rounds 1-5 of this tree: train(total_steps, ...) with the count first)
        if total_steps is None:
            raise TypeError("train(): total_steps is required (models.py:110)")
        del config
        save = (self.rank == 0) if save is None else bool(save)
        summarize = bool(save_summary_steps) and model_dir is not None
        self._keep_waveforms, self._real_waveforms = summarize, None
        writer = None
        if summarize and self.rank == 0:
            from . import summary
            writer = summary.SummaryWriter(model_dir)
        try:
            self._train_loop(model_dir, total_steps, save_checkpoint_steps, save_summary_steps if summarize else None, log_tensor_steps,
                             log, save, writer)
        finally:
            self._keep_waveforms, self._real_waveforms = False, None
            if writer is not None:
                writer.close()

    def _train_loop(self, model_dir, total_steps, save_checkpoint_steps, save_summary_steps, log_tensor_steps, log, save, writer):
        from . import checkpoint
        have = True
        if model_dir is not None and self.g_params is None:
            # the variables exist from step 0 in the reference's graph: build them from the first batch's shapes and restore BEFORE the
            # stop condition is looked at (a finished run resumes to zero further steps, not one)
            try:
                self._peeked = self._next_inputs()
            except StopIteration:
                have = False
            if self._all_ranks_have_input(have):
                _, labels, d_latents, _, _ = self._peeked
                self._ensure_built(d_latents, labels)
                self.restored_from = checkpoint.restore(self, model_dir)
            else:
                have, self._peeked = False, None
        elif model_dir is not None:
            self.restored_from = checkpoint.restore(self, model_dir)
        last_saved = None
        while have and self.global_step < total_steps:
            try:
                inputs = self._next_inputs()
            except StopIteration:
                inputs = None
            if not self._all_ranks_have_input(inputs is not None):
                break
            self._peeked = inputs
            d_loss, g_loss = self.train_step()
            if log is not None and self.global_step % log_tensor_steps == 0:
                log(f"global_step = {self.global_step}, generator_loss = {float(g_loss):.6f}, "
                    f"discriminator_loss = {float(d_loss):.6f}")
            if save_summary_steps and self.global_step % save_summary_steps == 0:
                self._join_updates()   # (every rank, as for the checkpoint below: it may be a collective)
                if writer is not None:
                    self._summarize(writer, inputs, d_loss, g_loss)
            if model_dir is not None and save_checkpoint_steps and self.global_step % save_checkpoint_steps == 0:
                # (global_step is the same on every rank.)  The pending generator update may still need its all-reduce: EVERY rank
                # joins here, so that the rank-local save below finds nothing left to communicate -- a collective issued by rank 0
                # alone would pair with its peers' NEXT all-reduce and leave the job one collective out of step for good.
                self._join_updates()
                if save:
                    last_saved = self.global_step
                    checkpoint.save(self, model_dir)
                if writer is not None:
                    writer.flush()
        if self.g_params is not None:
            self._join_updates()   # (every rank: the last generator update, and the final save must not communicate either)
        if model_dir is not None and save and self.g_params is not None and last_saved != self.global_step:
            checkpoint.save(self, model_dir)
        if writer is not None:
            writer.flush()

    def _summarize(self, writer, inputs, d_loss, g_loss):
        """One summary step (see train): the updates are joined; `inputs` are the iteration's own (_next_inputs)."""
        real_images, _, _, g_latents, g_labels = inputs
        step = self.global_step
        with torch.no_grad():
            fake_images = self.generator(g_latents, g_labels)
        audio = {}
        if self._real_waveforms is not None:
            audio["real_waveforms"] = self._real_waveforms
        if self.spectral_params is not None:
            audio["fake_waveforms"] = spectral_ops.convert_images_to_waveform(fake_images, **self.spectral_params)
        if audio:
            writer.audio(step, audio, self.spectral_params["sample_rate"] if self.spectral_params is not None else 16000)
        writer.images(step, {("real_magnitude_spectrograms", "real_instantaneous_frequencies"): real_images,
                             ("fake_magnitude_spectrograms", "fake_instantaneous_frequencies"): fake_images})
        writer.scalars(step, dict(generator_loss=float(g_loss), discriminator_loss=float(d_loss)))

    def generate(self, *args, **kwargs):
        """Two forms.
        `generate(model_dir, config)` -- the reference's (models.py:232-250, called at gan_synth_main.py:128-131): restores the latest
        checkpoint of `model_dir` (MonitoredSession semantics: the initial weights when there is none), then YIELDS one numpy batch of
        fake waveforms [B, waveform_length] per batch of the input functions -- labels of `real_input_fn()`, latents of
        `fake_input_fn()`, as models.py:22-31 wires `fake_waveforms` -- until the input runs dry (OutOfRangeError, :249).  `config`
        (tf.ConfigProto) is accepted and ignored.
        `generate(latents, labels)` -- fake waveforms (a device tensor) for one given batch.
        `weights` (keyword, both forms): "live" -- the weights as the last Adam step left them -- or "average": the averaged generator
        (averaged_generator(); the checkpoint is restored first, and a model built without generator_average_decay takes the averages
        from it: ValueError when there is nothing to take them from).  Data parallel: as every reader of the weights it joins the pending
        update first -- a collective when `collective_pending()`.
        `sample_rate` (keyword, both forms): None or the model's own rate -- the waveforms as generated; another rate -- every row
        resampled to it on the device (spectral_ops.resample: [B, ceil(waveform_length * sample_rate / model rate)]), not normalised:
        the reference writes raw floats."""
        if "model_dir" in kwargs or (args and (args[0] is None or isinstance(args[0], (str, bytes)) or hasattr(args[0], "__fspath__"))):
            return self._generate_from(*args, **kwargs)
        return self._generate_batch(*args, **kwargs)

    def _generate_from(self, model_dir, config=None, weights="live", sample_rate=None):
        del config
        restored = False
        while True:
            try:
                _, labels = self.real_input_fn()
            except StopIteration:
                return
            latents = self.fake_input_fn()
            dev = self.store.device if hasattr(self.store, "device") else labels.device
            latents, labels = latents.to(dev), labels.to(dev)
            self._ensure_built(latents.to(self.dtype), labels.to(self.dtype))
            if not restored:
                restored = True
                self.restored_from = self._restore_for(model_dir, weights)
            # (the swap there and back around EVERY batch: between two yields the caller finds the model as it always is)
            yield self._generate_batch(latents, labels, weights=weights, sample_rate=sample_rate).float().cpu().numpy()

    def _generate_batch(self, latents, labels, weights="live", sample_rate=None):
        """models.py:22-31 (`fake_waveforms`): fake waveforms for a batch."""
        if weights not in ("live", "average"):
            raise ValueError(f"weights must be 'live' or 'average' (got {weights!r})")
        if weights == "average" and not self._average_in:
            with self.averaged_generator():
                return self._generate_batch(latents, labels, sample_rate=sample_rate)
        self._join_updates()
        with torch.no_grad():
            images = self.generator(latents.to(self.dtype), labels.to(self.dtype))
        waves = spectral_ops.convert_images_to_waveform(images, **self.spectral_params)
        if sample_rate is None:
            return waves
        return spectral_ops.resample(waves, self.spectral_params["sample_rate"], sample_rate)

    # --------------------------------------------------------------------------------------- note sequences
    def synthesize(self, notes, model_dir=None, latents=None, seed=0, seconds_per_instrument=6.0, release_seconds=1.0, normalize=True,
                   want_pcm=False, info=None, pitches=range(24, 85), batch_size=8, weights="live", sample_rate=None, controllers=False,
                   controller_ramp=0.01, bend=False, sustain=False, ensemble=False, stereo=False, spread=0.0):
        """A score -> one mixed clip (not in the reference: the rules are this project's own, DESIGN.md "Note sequences").

        `notes`: notes.Note rows, or what notes.read_notes accepts (a .mid / .json file name or bytes).  Restores the latest checkpoint of
        `model_dir` as `generate` does (None: the weights as they are).  Every note whose pitch is in the label table sorted(`pitches`)
        is generated -- its latent by spherical interpolation between anchors `seconds_per_instrument` apart, drawn from a generator of
        their own seeded with `seed`, or from `latents` ([N, 256]: one row per kept note; [256]: one fixed instrument) -- in chunks of
        `batch_size` (the last one padded by repeating its last row, so that every note runs at the same batch size and tile choice),
        and all notes are mixed by ONE gs_note_mix call: held for their length, released linearly over `release_seconds`, scaled by
        velocity / 127, the clip divided by its peak when `normalize` and the peak exceeds 1.
        Returns the clip [T] fp32 on the device, or (clip, int16 clip) with `want_pcm`.  `info` (a dict) receives notes (the kept ones),
        dropped, total_samples, latents ([N, 256] fp32, host) and peak.  `weights`: "live" or "average", as for `generate`.  One process only.
        `sample_rate`: None or the model's own rate -- the clip as mixed.  Another rate (DESIGN.md "Output rates"): the mix is left
        unnormalised and without PCM, and ONE gs_resample call brings it to that rate, takes the peak THERE (a band-limited interpolation
        overshoots the samples it passes through), normalises by it and quantises; the clip (and PCM) come back at the new rate.  `info`
        also receives sample_rate and output_samples, and its peak is the resampled clip's; total_samples keeps its meaning at the
        model's rate.
        `ensemble`, `stereo`, `spread` (DESIGN.md "Parts and stereo"; all off: the path above, untouched).  With either flag the score is
        read by notes.read_score (a notes.Score is taken as it is, a list of Note is one part with the default volume and no pan).
        `ensemble`: every part -- a MIDI channel under one program, a JSON "part" -- plays its own instrument
        (notes.schedule_part_latents, unless `latents` is given) and the channel volume enters the gain, velocity * volume / 127^2.
        `stereo`: pan and `spread` (in [0, 1]: how far the parts without a pan fan out) enter the two gains of notes.schedule_gains, ONE
        gs_note_mix_stereo call mixes both channels and normalises them by their joint peak; the clip is [2, T] and the PCM [T, 2].  With
        `sample_rate` at another rate: the stereo mix unnormalised, ONE gs_resample call on its two rows, ONE gs_stereo_finish at the new
        rate.  `info` also receives parts, part_of_note (per kept note) and channels.
        `controllers`, `controller_ramp` (DESIGN.md "Controllers"; off: the paths above, untouched).  The score is read by
        notes.read_performance (a notes.Performance is taken as it is; a Score or a list of Note has no controls): the sustain pedal has
        moved note ends, and channel volume, expression and -- with `stereo` -- pan form one gain curve per part (notes.schedule_curves,
        every change a ramp of `controller_ramp` seconds).  A note's own gain is velocity / 127 and nothing else; ONE gs_note_mix_curves
        call takes the place of the gs_note_mix / gs_note_mix_stereo call and everything behind it is as above.  `ensemble` still decides
        the instruments only.  `info` also receives controls (counts by kind), pedal_extended and curve_points.
        `bend` (DESIGN.md "Pitch bend"; off, or on with a score that bends no note: the paths above, not a launch changed).  True: the
        score's pitch bend is read by notes.read_bends (a score given as notes.Note rows, a Score or a Performance carries none); or the
        bends themselves, per part a list of (seconds, semitones).  Each note's part is read_score's, whatever `ensemble`, `stereo` and
        `controllers` decide about instruments and gains.  Every part with a bend gets one playback-rate curve (notes.schedule_bends,
        every change a ramp of `controller_ramp` seconds); `waves` is allocated [N + B, L] for the B notes whose curve leaves 1 while
        they sound, the generator fills the first N rows, ONE gs_note_warp call writes the bent copies into the rest, the bent notes'
        table rows name their copies, and the chosen mix call and everything behind it run unchanged.  The clip's length and every
        onset stay as they are.  `info` also receives bends (events per part), bent_notes and bend_points.
        `sustain` (DESIGN.md "Sustain"; off, or on with a score whose every note fits the waveform with its release: the paths above,
        not a launch, a table row or an output bit changed).  True: a note with hold + R > L (notes.schedule_sustain: the hold unclamped,
        R the full release) is HELD -- it sounds for its whole length and keeps its whole release.  `waves` is allocated with one more
        row per piece of a held note (pieces of at most L samples), ONE gs_loop_search call scores the loop lengths of the held notes'
        generated rows under notes.sustain_plan(L), notes.pick_loop picks one per note on the host, ONE gs_note_sustain call writes the
        pieces of the looped waveform into the extra rows, and the chosen mix call and everything behind it run unchanged on a table
        that holds one entry per piece; the clip grows to the score's length.  Bend and sustain do not compose -- a bent piece would
        have to start reading where the earlier pieces stopped, and gs_note_warp has no such start: a held note whose part bends while
        it sounds is cut at L as before and counted.  `info` also receives held_notes, sustain_rows, loops (per held note
        (a, m, score)) and sustain_cut_bent."""
        from . import notes as N
        if self.world > 1:
            raise RuntimeError("GANSynth.synthesize runs in one process: launch it without torch.distributed (world size 1)")
        if self.spectral_params is None:
            raise ValueError("synthesize: the model has no spectral_params (waveform_length, sample_rate, ...)")
        score = performance = bends = None
        if isinstance(bend, (list, tuple)):
            bends, bend = [list(events) for events in bend], True
        is_rows = isinstance(notes, (list, tuple)) and all(isinstance(n, N.Note) for n in notes)
        if bend and bends is None and not is_rows and not isinstance(notes, (N.Score, N.Performance)):
            if not isinstance(notes, (bytes, bytearray, memoryview)):
                with open(os.fspath(notes), "rb") as f:   # (read once: the readers below take the bytes)
                    notes = f.read()
            bends = N.read_bends(notes)
        if bends is not None:   # (refusals first)
            bend_points, bend_first = N.schedule_bends(bends, self.spectral_params["sample_rate"], controller_ramp)
        bend_counts = [len(events) for events in bends] if bends is not None else []
        if bends is not None and not any(bends):
            bends = None                                   # a score without a bend: the paths as they are
        bend_score = None
        if bends is not None and not (controllers or ensemble or stereo):   # the parts, for the plain path: read_score's
            bend_score = notes if isinstance(notes, N.Score) else N.one_part_score(notes) if is_rows else \
                notes.score if isinstance(notes, N.Performance) else N.read_score(notes)
            notes = bend_score.notes
        if controllers:
            if isinstance(notes, N.Performance):
                performance = notes
            elif isinstance(notes, N.Score):
                performance = N.plain_performance(notes)
            elif isinstance(notes, (list, tuple)) and all(isinstance(n, N.Note) for n in notes):
                performance = N.plain_performance(N.one_part_score(notes))
            else:
                performance = N.read_performance(notes)
            score = performance.score
            notes = score.notes
            N.schedule_curves(performance, [], self.spectral_params["sample_rate"], controller_ramp, stereo, spread)   # (refusals first)
        elif ensemble or stereo:
            if isinstance(notes, N.Score):
                score = notes
            elif isinstance(notes, (list, tuple)) and all(isinstance(n, N.Note) for n in notes):
                score = N.one_part_score(notes)
            else:
                score = N.read_score(notes)
            notes = score.notes
            N.part_positions(score, spread)   # (a spread outside [0, 1] is refused before anything is generated)
        elif not (isinstance(notes, (list, tuple)) and all(isinstance(n, N.Note) for n in notes)):
            notes = N.read_notes(notes)
        pitches = sorted(pitches)
        sr, length = self.spectral_params["sample_rate"], int(self.spectral_params["waveform_length"])
        kept, table, total, dropped = N.schedule(notes, pitches, sr, length, release_seconds)
        count, batch = len(kept), int(batch_size)
        held, cut_bent = [], 0
        if sustain:   # which notes are held, and how long the clip becomes; the pieces enter the table once it has its gains
            _, piece_table, piece_total, _, owner, offsets = N.schedule_sustain(notes, pitches, sr, length, release_seconds)
            held = sorted({n for n, offset in zip(owner, offsets) if offset is not None})
            parts = score if score is not None else bend_score
            if held and bends is not None and len(bends) == len(parts.parts):   # (another count is refused below)
                index = N.kept_indices(notes, pitches)
                spans = {n: [table[n][0], 0, N._round(release_seconds * sr)] for n in held}   # the whole span of a held note
                for row, n, offset in zip(piece_table, owner, offsets):
                    if offset is not None:
                        spans[n][1] += row[1]
                bent = N.bent_notes([spans[n] for n in held], [parts.part[index[n]] for n in held], bend_points, bend_first)
                if bent:   # bend and sustain do not compose: these are cut at L, as without the flag
                    cut_bent = len(bent)
                    _, piece_table, piece_total, _, owner, offsets = N.schedule_sustain(notes, pitches, sr, length, release_seconds,
                                                                                        cut=[held[i] for i in bent])
                    held = [n for i, n in enumerate(held) if i not in set(bent)]
            if held:
                total = piece_total
                sustain_plan = N.sustain_plan(length)   # (a waveform too short to loop is refused before anything is generated)
        if score is not None:
            index = N.kept_indices(notes, pitches)
            part_of_note = [score.part[i] for i in index]
        if performance is not None:   # velocity / 127 and the part: volume, expression and pan reach the samples through the curves
            table = [row + (part,) for row, part in zip(table, part_of_note)]
            points, first = N.schedule_curves(performance, index, sr, controller_ramp, stereo, spread)
        elif score is not None:
            if not ensemble:   # one instrument, and the channel volume does not enter: 127 / 127 is an exact 1
                score = score._replace(volume=[127] * len(score.notes))
            if stereo:
                table = [row[:4] + gains for row, gains in zip(table, N.schedule_gains(index, score, spread))]
            else:
                table = [row[:4] + (score.notes[i].velocity * score.volume[i] / 127.0 ** 2,) for row, i in zip(table, index)]
        if latents is None and ensemble:
            lat = N.schedule_part_latents(kept, part_of_note, len(score.parts), total, sr, seed, seconds_per_instrument)
        elif latents is None:
            lat = N.schedule_latents(kept, total, sr, seed, seconds_per_instrument)
        else:
            lat = torch.as_tensor(latents).detach().float().cpu()
            if lat.dim() == 1:
                lat = lat[None].expand(count, -1)
            if lat.dim() != 2 or lat.shape[0] != count:
                raise ValueError(f"synthesize: latents must be [{count}, Z] (one row per kept note) or [Z] (got {tuple(lat.shape)})")
            lat = lat.contiguous()
        warp_notes = []
        if bends is not None:   # the bent notes get rows of their own behind the generated ones
            parts = score if score is not None else bend_score
            if len(bends) != len(parts.parts):
                raise ValueError(f"synthesize: bend must hold one list of events per part of the score, {len(parts.parts)} (got {len(bends)})")
            bend_part = [parts.part[i] for i in N.kept_indices(notes, pitches)]
            curved = [p for p in range(len(bends)) if bend_first[p] < bend_first[p + 1]]
            for n in N.bent_notes(table, bend_part, bend_points, bend_first):
                onset, hold, release, row = table[n][:4]
                warp_notes.append((row, count + len(warp_notes), onset, hold + release, curved.index(bend_part[n])))
                table[n] = table[n][:3] + (count + len(warp_notes) - 1,) + table[n][4:]
        pieces = []   # (held note, its row behind the generated and the bent ones, offset into the note, samples)
        if held:      # a held note's entry becomes one entry per piece, with the note's gains (and curve)
            per_note, table = table, []
            for row, n, offset in zip(piece_table, owner, offsets):
                if offset is None:
                    table.append(per_note[n])
                    continue
                table.append(row[:3] + (count + len(warp_notes) + len(pieces),) + per_note[n][4:])
                pieces.append((n, count + len(warp_notes) + len(pieces), offset, row[1] + row[2]))
        labels = N.labels_for(kept, pitches)
        dev = self.store.device if hasattr(self.store, "device") else "cuda"
        if self.g_params is None:
            self._build(lat[:1].expand(batch, -1).to(dev, self.dtype), labels[:1].expand(batch, -1).to(dev, self.dtype))
        restored = self._restore_for(model_dir, weights)
        if model_dir is not None:
            self.restored_from = restored
        self._join_updates()
        waves = torch.empty((count + len(warp_notes) + len(pieces), length), dtype=torch.float32, device=dev)
        with self.averaged_generator() if weights == "average" else contextlib.nullcontext():
            for lo in range(0, count, batch):
                rows = [min(i, count - 1) for i in range(lo, lo + batch)]   # the last chunk repeats its last row
                wave = self._generate_batch(lat[rows].to(dev), labels[rows].to(dev))
                waves[lo:min(lo + batch, count)].copy_(wave[:min(batch, count - lo)])   # (the rows behind `count` are the bent copies')
        # mix, then resample if asked, then (two resampled channels) the joint finish: only the last stage normalises and quantises
        K = kernels.get()
        if warp_notes:
            K.note_warp(waves, warp_notes, bend_points, [bend_first[p] for p in curved] + [len(bend_points)])
        loops = []
        if held:   # score the loop lengths on the device, pick on the host, write the pieces of the looped notes
            loop_a, m_min, _, _, xfade = sustain_plan
            scores = K.loop_search(waves, held, sustain_plan).cpu().numpy()
            picked = {n: N.pick_loop(scores[i], m_min) for i, n in enumerate(held)}
            loops = [(loop_a, picked[n], float(scores[i, picked[n] - m_min])) for i, n in enumerate(held)]
            K.note_sustain(waves, [(n, row, offset, samples, loop_a, picked[n], xfade) for n, row, offset, samples in pieces])
        resampled = sample_rate is not None and int(sample_rate) != int(sr)
        last, unfinished = dict(normalize=normalize, want_pcm=want_pcm), dict(normalize=False, want_pcm=False)
        if performance is not None:
            clip, pcm, peak = K.note_mix_curves(waves, table, points, first, total, channels=2 if stereo else 1, **(unfinished if resampled else last))
        else:
            clip, pcm, peak = (K.note_mix_stereo if stereo else K.note_mix)(waves, table, total, **(unfinished if resampled else last))
        if resampled:
            clip, pcm, peak = K.resample(clip, int(sr), int(sample_rate), **(unfinished if stereo else last))
            if stereo:
                clip, pcm, peak = K.stereo_finish(clip, **last)
            else:
                clip, pcm = clip[0], (pcm[0] if want_pcm else None)
        if info is not None:
            info.update(notes=kept, dropped=dropped, total_samples=total, latents=lat, peak=float(peak),
                        sample_rate=int(sr if sample_rate is None else sample_rate), output_samples=int(clip.shape[-1]))
            if score is not None:
                info.update(parts=list(score.parts), part_of_note=part_of_note, channels=2 if stereo else 1)
            if performance is not None:
                info.update(controls=N.control_counts(performance), pedal_extended=performance.pedal_extended, curve_points=len(points))
            if bend:
                info.update(bends=bend_counts, bent_notes=len(warp_notes),
                            bend_points=len(bend_points) if bends is not None else 0)
            if sustain:
                info.update(held_notes=len(held), sustain_rows=len(pieces), loops=loops, sustain_cut_bent=cut_bent)
        return (clip, pcm) if want_pcm else clip

    # ------------------------------------------------------------------------------------------- evaluation
    def evaluate(self, model_dir, config, classifier, input_name="images:0", output_names=("features:0", "logits:0"), batch_size=64,
                 extra_metrics=False, classifier_dtype=torch.float32, features_out=None, weights="live", ndb="sklearn", swd=False, swd_seed=0, prd=False, prd_k=3,
                 f0=False, pitches=range(24, 85), kid=False, kid_subsets=100, kid_subset_size=1000, kid_seed=0):
        """models.py:196-230: the Frechet distance between the pitch classifier's features of real and generated spectrograms.

        Restores the latest checkpoint of `model_dir` as `generate` does, then for every batch of `real_input_fn()` until it runs dry:
        real images from its waveforms (the spectral kernels), fake images from `fake_input_fn()` latents with THAT batch's labels
        (models.py:22-27); both go through the classifier in batches of `batch_size` (independent of the GAN's batch).
        `classifier`: a networks.ResNet, or its weights (a frozen GraphDef path or bytes, a .safetensors path) for the reference's
        pitch classifier.  `input_name` / `output_names` must name the reference graph's tensors ("images:0", then "features:0" and
        "logits:0").  `config` (tf.ConfigProto) is accepted and ignored.  Returns {"frechet_inception_distance": float}; with
        `extra_metrics` also the inception score of the fake logits, the pitch accuracy of their argmax against the conditioning labels
        and, when scikit-learn imports, the number of statistically different bins.  `features_out` (a dict): receives the host arrays
        real_features, fake_features, real_logits, fake_logits, labels.  `weights`: "live" or "average", as for `generate` -- the fake side
        comes from the averaged generator, swapped in behind the restore and out again at the end.  `ndb` (read with `extra_metrics`):
        "sklearn" as above; "device": num_different_bins and bin_jsd (the Jensen-Shannon divergence of the bin proportions) from
        metrics.num_different_bins_device -- k-means on HIP kernels, no scikit-learn.  `swd`: the dict gains sliced_wasserstein_distance (the
        mean over the levels) and sliced_wasserstein_distance_levels (a list, finest first; features_out receives their sizes as swd_sizes,
        "HxW" a level): the sliced Wasserstein distance between Laplacian-pyramid patches of the same real and fake images (swd.py: HIP
        kernels, corners and directions seeded by `swd_seed`), every batch added as it arrives -- the images are not kept.  `classifier` may
        be None together with `swd`: no classifier is loaded or run and only the two SWD keys come back.  `prd`: the dict gains precision,
        recall, density and coverage of the fake features against the real ones -- the features of the FID -- from
        metrics.precision_recall_device (manifold.py: `prd_k`-nearest-neighbour radii on HIP kernels); it needs the classifier.  `f0`: pitch from
        the AUDIO, without a classifier (pitch.py: a YIN f0 tracker on HIP kernels, DESIGN.md "Pitch tracking on the device").  Every batch's real
        waveforms (the data itself where it is waveforms, else the images through convert_images_to_waveform) and the generated images through the
        inverse transform `generate` uses are tracked and judged against THAT batch's labels -- a label index is a MIDI pitch through
        sorted(`pitches`), the list `synthesize` gets -- note by note as the batches arrive; the waveforms are not kept.  The dict gains, for the
        generated side, f0_pitch_accuracy (the share of notes whose median deviation from the label is under 50 cents), f0_chroma_accuracy (the same
        with the cents folded to +-600: octave errors are the gap between the two), f0_median_abs_cents and f0_jitter_cents (the mean within-note
        standard deviation), both over the notes counted accurate, and f0_voiced_fraction; and the same five with the prefix real_.  YIN is not
        perfect on real instruments (bass notes, mallets): the real_ figures are the calibration the generated ones are read against.
        features_out receives real_f0_cents and fake_f0_cents (one a note, NaN for an unvoiced one).  `classifier` may be None together with `swd`
        or `f0`.  `kid`: the dict gains kernel_inception_distance -- the unbiased estimate of the squared maximum mean discrepancy between the
        fake and the real features (the features of the FID) under the cubic kernel, over all rows; unlike the Frechet distance its expectation does
        not depend on the number of notes, and it may be negative -- and kernel_inception_distance_subset_mean / _subset_std, its mean and
        population standard deviation over `kid_subsets` subsets of min(`kid_subset_size`, rows) rows a side drawn with `kid_seed`, from
        metrics.kernel_inception_distance_device (kid.py: an fp64 matrix-core HIP kernel, DESIGN.md "KID on the device"); it needs the classifier.
        features_out receives kid_subset_values (one estimate a subset).  One process only."""
        import numpy as np
        from . import metrics, networks
        del config
        if ndb not in ("sklearn", "device"):
            raise ValueError(f"evaluate: ndb must be 'sklearn' or 'device' (got {ndb!r})")
        if self.world > 1:
            raise RuntimeError("GANSynth.evaluate runs in one process: launch it without torch.distributed (world size 1)")
        if input_name != "images:0" or list(output_names) != ["features:0", "logits:0"]:
            raise ValueError(f"evaluate: the classifier graph's tensors are 'images:0' -> ['features:0', 'logits:0'] "
                             f"(got {input_name!r} -> {list(output_names)!r})")
        if classifier is None and prd:
            raise ValueError("evaluate: prd=True needs a classifier (precision, recall, density and coverage come from its features)")
        if prd and (not isinstance(prd_k, int) or isinstance(prd_k, bool) or not 1 <= prd_k <= 8):   # (before the first batch, not after the last)
            raise ValueError(f"evaluate: prd_k must be an integer in [1, 8] (got {prd_k!r})")
        if classifier is None and kid:
            raise ValueError("evaluate: kid=True needs a classifier (the kernel inception distance comes from its features)")
        if kid:   # (before the first batch, not after the last)
            for name, v, low in (("kid_subsets", kid_subsets, 0), ("kid_subset_size", kid_subset_size, 2)):
                if not isinstance(v, int) or isinstance(v, bool) or v < low:
                    raise ValueError(f"evaluate: {name} must be an integer >= {low} (got {v!r})")
        if classifier is None:
            if not swd and not f0:
                raise ValueError("evaluate: classifier=None needs swd=True or f0=True (every other figure comes from the pitch classifier)")
            resnet = None
        elif isinstance(classifier, networks.ResNet):
            resnet = classifier
        else:
            resnet = networks.ResNet.pitch_classifier().load(classifier)
        sliced = None
        tracked = None
        if f0:
            from . import pitch
            table = np.asarray(sorted(pitches), dtype=np.float64)
            tracked = {"real": pitch.NoteAccumulator(rate=self.spectral_params["sample_rate"]), "fake": pitch.NoteAccumulator(rate=self.spectral_params["sample_rate"])}
        real_f, fake_f, real_l, fake_l, labs = [], [], [], [], []
        pending = {"real": [], "fake": []}

        def flush(which, force=False):
            while pending[which] and (force or sum(t.shape[0] for t in pending[which]) >= batch_size):
                x = torch.cat(pending[which])
                take, rest = x[:batch_size], x[batch_size:]
                pending[which] = [rest] if rest.shape[0] else []
                f, l = resnet(take.to(classifier_dtype).contiguous(memory_format=torch.channels_last))
                (real_f if which == "real" else fake_f).append(f.cpu().numpy())
                (real_l if which == "real" else fake_l).append(l.cpu().numpy())

        restored = False
        with contextlib.ExitStack() as swapped:   # (the average goes in behind the restore of the first batch, out at the end)
            while True:
                try:
                    data, labels = self.real_input_fn()
                except StopIteration:
                    break
                latents = self.fake_input_fn()
                dev = self.store.device if hasattr(self.store, "device") else labels.device
                data, latents, labels = data.to(dev), latents.to(dev), labels.to(dev)
                self._ensure_built(latents.to(self.dtype), labels.to(self.dtype))
                if not restored:
                    restored = True
                    self.restored_from = self._restore_for(model_dir, weights)
                    if weights == "average":
                        swapped.enter_context(self.averaged_generator())
                self._join_updates()
                with torch.no_grad():
                    real = spectral_ops.convert_to_images(data, **self.spectral_params, dtype=self.dtype) if data.dim() == 2 else data
                    fake = self.generator(latents.to(self.dtype), labels.to(self.dtype))
                if swd:
                    if sliced is None:
                        from . import swd as swd_module
                        sliced = swd_module.SlicedWasserstein(real.shape, seed=swd_seed)
                    sliced.add(real, fake)
                if f0:
                    if labels.shape[1] != len(table):
                        raise ValueError(f"evaluate: f0=True reads a label index as a pitch: {labels.shape[1]} label columns, {len(table)} pitches")
                    note_pitches = table[labels.argmax(dim=1).cpu().numpy()]
                    tracked["real"].add(data if data.dim() == 2 else spectral_ops.convert_images_to_waveform(data, **self.spectral_params), note_pitches)
                    tracked["fake"].add(spectral_ops.convert_images_to_waveform(fake, **self.spectral_params), note_pitches)
                if resnet is None:
                    continue
                pending["real"].append(real)
                pending["fake"].append(fake)
                labs.append(labels.float().cpu().numpy())
                flush("real")
                flush("fake")
        if not restored:
            raise ValueError("evaluate: real_input_fn() gave no batch")
        sliced_out = {}
        if swd:
            result = sliced.result()
            sliced_out = dict(sliced_wasserstein_distance=result["mean"], sliced_wasserstein_distance_levels=result["levels"])
            if features_out is not None:
                features_out.update(swd_sizes=result["sizes"])
        if f0:
            for which, prefix in (("fake", ""), ("real", "real_")):
                figures, cents, _ = tracked[which].result()
                sliced_out.update({prefix + key: value for key, value in figures.items()})
                if features_out is not None:
                    features_out[which + "_f0_cents"] = cents
        if resnet is None:
            return sliced_out
        flush("real", True)
        flush("fake", True)
        real_f, fake_f = np.concatenate(real_f), np.concatenate(fake_f)
        real_l, fake_l, labs = np.concatenate(real_l), np.concatenate(fake_l), np.concatenate(labs)
        if features_out is not None:
            features_out.update(real_features=real_f, fake_features=fake_f, real_logits=real_l, fake_logits=fake_l, labels=labs)
        out = dict(frechet_inception_distance=metrics.frechet_inception_distance(real_f, fake_f))
        if extra_metrics:
            out["inception_score"] = metrics.inception_score(fake_l)
            out["pitch_accuracy"] = float(np.mean(np.argmax(fake_l, axis=1) == np.argmax(labs, axis=1)))
            if ndb == "device":
                details = {}
                out["num_different_bins"] = metrics.num_different_bins_device(real_f, fake_f, details=details)
                out["bin_jsd"] = details["jsd"]
            else:
                try:
                    out["num_different_bins"] = metrics.num_different_bins(real_f, fake_f, random_state=0)
                except ImportError:
                    pass
        if prd:
            out.update(metrics.precision_recall_device(real_f, fake_f, k=prd_k))
        if kid:
            details = {}
            out.update(metrics.kernel_inception_distance_device(real_f, fake_f, subsets=kid_subsets, subset_size=kid_subset_size, seed=kid_seed, details=details))
            if features_out is not None:
                features_out.update(kid_subset_values=details["subset_kids"])
        out.update(sliced_out)
        return out


def exponential_decay(learning_rate, global_step, decay_steps, decay_rate):
    """tf.train.exponential_decay, staircase=False: learning_rate * decay_rate ** (global_step / decay_steps)."""
    return float(learning_rate) * float(decay_rate) ** (float(global_step) / float(decay_steps))


class PitchClassifier(object):
    """models.py:253-408: the pitch classifier's training and evaluation.  `network`: a networks.ResNet; `input_fn()` -> (waveforms
    [B, L] or images [B, 2, T, F], one-hot labels [B, classes]) until StopIteration; `hyper_params`: weight_decay, learning_rate (a
    float or a callable of the global step), momentum, use_nesterov (pitch_classifier_main.py:71-81).

    Training (fp32 activations) is softmax cross-entropy + weight_decay * sum(v^2) / 2 over every variable whose name does not contain
    "normalization", minimised by tf.train.MomentumOptimizer: networks.ResNet.forward_backward and .momentum_step, all on HIP kernels.
    Checkpoints are .safetensors files (classifier_io.write_safetensors) named like checkpoint.py's: the variables under their reference
    names, the momentum accumulators under "momentum/<variable>" and "global_step" -- nothing but the variables starts with "resnet/",
    so a checkpoint is itself a classifier weight file (GANSynth.evaluate's `classifier`, gan_synth_main.py --classifier)."""

    SLOT_PREFIX = "momentum/"
    MAX_TO_KEEP = 10   # tf.train.Saver(max_to_keep=10), models.py:322-325

    def __init__(self, network, input_fn, spectral_params, hyper_params=None, dtype=torch.float32):
        self.network, self.input_fn = network, input_fn
        self.spectral_params, self.hyper_params = spectral_params, hyper_params
        self.dtype = dtype
        self.global_step = 0
        self.restored_from = None

    def _images(self, data, dtype):
        data = data.to(self.network.store.device)
        with torch.no_grad():
            images = spectral_ops.convert_to_images(data, **self.spectral_params, dtype=dtype) if data.dim() == 2 else data
        return images.to(dtype).contiguous(memory_format=torch.channels_last)

    # ------------------------------------------------------------------------------------------------ checkpoints
    @classmethod
    def slot_name(cls, variable):
        """Checkpoint key of a variable's momentum accumulator."""
        return cls.SLOT_PREFIX + variable

    @classmethod
    def split_state(cls, state):
        """A checkpoint's entries -> ({variable: array}, {variable: its accumulator}, global_step or None)."""
        import numpy as np
        slots = {k[len(cls.SLOT_PREFIX):]: v for k, v in state.items() if k.startswith(cls.SLOT_PREFIX)}
        weights = {k: v for k, v in state.items() if not k.startswith(cls.SLOT_PREFIX) and k != "global_step"}
        return weights, slots, (int(np.asarray(state["global_step"]).reshape(-1)[0]) if "global_step" in state else None)

    def state_dict(self):
        """{name: host array}: variables, "momentum/<variable>" accumulators, "global_step"."""
        st = self.network.train_state()
        torch.cuda.synchronize()
        out = {}
        for name, p in st.flat.named.items():
            out[name] = p.data.detach().cpu().numpy().copy()
        for name, p in st.flat.named.items():
            off = (p.data.data_ptr() - st.flat.flat.data_ptr()) // 4
            out[self.slot_name(name)] = st.flat.m[off:off + p.numel()].view(p.shape).cpu().numpy().copy()
        import numpy as np
        out["global_step"] = np.asarray(self.global_step, dtype=np.int64)
        return out

    def save(self, model_dir):
        import glob
        import re
        from . import classifier_io
        os.makedirs(model_dir, exist_ok=True)
        path = os.path.join(model_dir, f"model.ckpt-{self.global_step}.safetensors")
        classifier_io.write_safetensors(path, self.state_dict())
        with open(os.path.join(model_dir, "checkpoint"), "w") as f:
            f.write(f'model_checkpoint_path: "{os.path.basename(path)}"\n')
        old = sorted(glob.glob(os.path.join(model_dir, "model.ckpt-*.safetensors")), key=lambda q: int(re.findall(r"ckpt-(\d+)", q)[-1]))
        for q in old[:-self.MAX_TO_KEEP]:
            os.remove(q)
        return path

    def restore(self, model_dir_or_file):
        """Variables, accumulators and global_step from a checkpoint file or the latest one of a directory; returns its path, or None
        when the directory has none (a fresh run)."""
        from . import checkpoint, classifier_io
        path = model_dir_or_file if os.path.isfile(model_dir_or_file) else checkpoint.latest(model_dir_or_file)
        if path is None:
            return None
        state = classifier_io.read_safetensors(path)
        st = self.network.train_state()
        weights, slots, step = self.split_state(state)
        self.network.load_state_dict(weights, strict=True)
        with torch.no_grad():
            st.flat.m.zero_()   # (a plain weight file: fresh accumulators)
            for name, p in st.flat.named.items():
                if name in slots:
                    if tuple(slots[name].shape) != tuple(p.shape):
                        raise ValueError(f"checkpoint: {self.slot_name(name)} has shape {tuple(slots[name].shape)}, the variable has {tuple(p.shape)}")
                    off = (p.data.data_ptr() - st.flat.flat.data_ptr()) // 4
                    st.flat.m[off:off + p.numel()].view(p.shape).copy_(torch.from_numpy(slots[name].copy()))
        self.global_step = step or 0
        return path

    # --------------------------------------------------------------------------------------------------- training
    def train(self, model_dir, config, total_steps, save_checkpoint_steps, save_summary_steps, log_tensor_steps, log=print):
        """models.py:306-386 with the reference's signature and argument order.  `config` (tf.ConfigProto) is accepted and ignored, as
        GANSynth.train does.  Resumes from the latest checkpoint of `model_dir`, steps until global_step reaches `total_steps` or the
        input runs dry, logs global_step, loss (cross-entropy + L2 term, at the pre-update weights) and accuracy (tf.metrics.accuracy:
        cumulative correct / total since this call began) every `log_tensor_steps`, saves every `save_checkpoint_steps` and at the end.
        `save_summary_steps` (when truthy and `model_dir` is given): the SummarySaverHooks of models.py:327-367 -- whenever
        global_step % save_summary_steps == 0 after a step, audio `waveforms` (when the input gave waveforms), images
        `magnitude_spectrograms` and `instantaneous_frequencies` and scalars `loss` and `accuracy` (the log line's values) of the step's
        own batch, into the events file of `model_dir`; by the modulus rule alone (TF's hook also fires on the first run of a session),
        flushed at every checkpoint and at the end."""
        del config
        net = self.network
        if self.dtype != torch.float32:
            raise TypeError("PitchClassifier.train: training runs in fp32 (bf16 training is not implemented)")
        net.train_state()
        if model_dir is not None:
            self.restored_from = self.restore(model_dir)
        writer = None
        if save_summary_steps and model_dir is not None:
            from . import summary
            writer = summary.SummaryWriter(model_dir)
        try:
            return self._train_loop(model_dir, total_steps, save_checkpoint_steps, save_summary_steps, log_tensor_steps, log, writer)
        finally:
            if writer is not None:
                writer.close()

    def _train_loop(self, model_dir, total_steps, save_checkpoint_steps, save_summary_steps, log_tensor_steps, log, writer):
        hp, net = self.hyper_params, self.network
        correct, total, last_saved = None, 0, None
        while self.global_step < total_steps:
            try:
                data, labels = self.input_fn()
            except StopIteration:
                break
            images = self._images(data, torch.float32)
            lr = hp.learning_rate(self.global_step) if callable(hp.learning_rate) else hp.learning_rate
            loss, hits, _, _ = net.forward_backward(images, labels)
            l2 = net.momentum_step(float(lr), hp.momentum, hp.use_nesterov, hp.weight_decay)
            self.global_step += 1
            correct = hits.to(torch.int64) if correct is None else correct + hits
            total += int(labels.shape[0])
            if log is not None and log_tensor_steps and self.global_step % log_tensor_steps == 0:
                log(f"global_step = {self.global_step}, loss = {float(loss) + float(hp.weight_decay) * float(l2):.6f}, "
                    f"accuracy = {int(correct) / max(total, 1):.6f}")
            if writer is not None and self.global_step % save_summary_steps == 0:
                step = self.global_step
                if data.dim() == 2:
                    writer.audio(step, dict(waveforms=data), self.spectral_params["sample_rate"])
                writer.images(step, {("magnitude_spectrograms", "instantaneous_frequencies"): images})
                writer.scalars(step, dict(loss=float(loss) + float(hp.weight_decay) * float(l2), accuracy=int(correct) / max(total, 1)))
            if model_dir is not None and save_checkpoint_steps and self.global_step % save_checkpoint_steps == 0:
                last_saved = self.global_step
                self.save(model_dir)
                if writer is not None:
                    writer.flush()
        if model_dir is not None and last_saved != self.global_step:
            self.save(model_dir)
        if writer is not None:
            writer.flush()
        return dict(global_step=self.global_step, accuracy=(int(correct) / max(total, 1)) if total else None)

    def evaluate(self, model_dir=None, config=None):
        """models.py:388-408: top-1 accuracy over the whole input.  `model_dir`: a training directory (its latest checkpoint is loaded),
        or classifier weights as a file (a frozen GraphDef or a .safetensors file), or None for the network's current weights.
        `config` is accepted and ignored."""
        del config
        if model_dir is not None:
            if os.path.isdir(model_dir):
                from . import checkpoint
                path = checkpoint.latest(model_dir)
                if path is None:
                    raise FileNotFoundError(f"PitchClassifier.evaluate: no checkpoint in {model_dir}")
                model_dir = path
            self.network.load(model_dir)
        correct, total = 0, 0
        while True:
            try:
                data, labels = self.input_fn()
            except StopIteration:
                break
            images = self._images(data, self.dtype)
            with torch.no_grad():
                _, logits = self.network(images)
            correct += int((logits.argmax(dim=1).cpu() == labels.argmax(dim=1).cpu()).sum())
            total += labels.shape[0]
        return dict(accuracy=correct / max(total, 1))
