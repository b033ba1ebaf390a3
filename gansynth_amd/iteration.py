"""The three ways the trainer runs an iteration under hipGraph replay, on the one capture mechanism of capture.py.  train_step asks in this order:

  form (graphs per iteration)    step / captures in                        runs when
  pipelined (4)                  _train_step_pipelined / _capture_pair     `_pipelined_ok`: `_graphable`, and `_overlap_in_graph`: data parallel on the library's own
                                                                           RCCL communicator, in-graph collectives not refused, GS_OVERLAP_REDUCE=1
  merged pair (2), or the whole  _train_step_merged / _capture_merged      `_merged_ok`: `_graphable`, forked branches, fused losses, the HIP library, GS_NO_MERGED_RUNS
  iteration as ONE graph (1):                                              unset; data parallel only with the all-reduce captured as the last node of a graph.
  the default                                                              One graph when `_fused_ok`: GS_NO_FUSED_ITERATION unset, gs_adam_tf_step_dev present
  one graph per run (2)          _plain_iteration / _run                   otherwise, and where all ranks fall back to together when a capture refuses its collective
                                                                           (capture._capture_agreed); `_run` launches eagerly when not `_graphable`

`Iterations` is a mix-in of models.GANSynth: the passes being captured (_part_a, _part_b, _forward_backward) are the trainer's.
"""
import contextlib
import warnings

import torch

from . import functional as F
from . import kernels
from .capture import _copy_inputs


class Iterations(object):

    def _graphable(self):
        """hipGraph replay needs a step-invariant launch sequence: the network structure is fixed within a growing regime (head
        depth, faded or not -- graphs are re-captured when it changes) and the one per-step scalar, the fade-in weight, is read
        from device memory (functional.DeviceLerp)."""
        return self.use_graphs and torch.cuda.is_available() and self._regime() is not None

    def _with_collective(self):
        """The run's gradient all-reduce goes into its captured graph: same-stream RCCL is capturable."""
        return self.distributed and self._comm is not None and self._graph_allreduce

    def _params_of(self, which):
        return self.d_params if which == "d" else self.g_params

    # ----------------------------------------------------------------------- one graph per run
    def _run(self, which, *inputs):
        self._join_updates()
        self._run_reduced = False
        if not self._graphable():
            self._graphs.clear()
            with self._stream_guard() if self.fork_eager else contextlib.nullcontext():
                return self._forward_backward(which, *inputs)
        head, fade = self._regime()
        key = (head, fade is None)
        if self._graph_key != key:
            self._drop_captures(new_regime=True)
            self._graph_key = key
        self._set_fade(fade)
        entry = self._graphs.get(which)
        if self._stale(entry, inputs):
            self._check_fork_runtime()
            entry = self._graphs[which] = self._capture_run(which, inputs)
        self._arm(self._params_of(which))
        _copy_inputs(entry["static"], inputs)
        entry["graph"].replay()
        self._run_reduced = entry["reduced"]   # (the replay already summed the gradients over the ranks: _apply goes straight to the update)
        return entry["loss"]

    def _capture_run(self, which, inputs):
        static = [t.detach().clone() for t in inputs]
        params = self._params_of(which)

        def capture(with_collective):
            graph = torch.cuda.CUDAGraph()
            with self._capturing_into(graph, with_collective=with_collective):
                return graph, self._forward_backward(which, *static)

        with self._capture_session():
            with_collective = self._with_collective()
            self._warm_up(lambda: self._forward_backward(which, *static), reduce=[params] if with_collective else [], clear=[params])
            # (refused on some rank: every rank captures the run again without the collective)
            graph, loss = self._capture_agreed(lambda: capture(with_collective), with_collective, abandon=(which,)) or capture(False)
        return self._record(static, graph=graph, loss=loss, reduced=self._captured_reduce)

    def _plain_iteration(self, d_latents, d_labels, real_images, g_latents, g_labels):
        """One graph per run (or none): the form every other one falls back to."""
        d_loss = self.discriminator_step(d_latents, d_labels, real_images)
        g_loss = self.generator_step(g_latents, g_labels)
        return d_loss, g_loss

    # ------------------------------------------------------------------ pipelined iteration
    # Data parallel, opt-in (GS_OVERLAP_REDUCE=1): every run as TWO graphs, part A (own network only) and part B (the rest), so that the
    # optimizer update of the OTHER network -- its gradient all-reduce above all -- can sit between them:
    #     D.A | update G | D.B | G.A | update D | G.B
    # Part A needs neither the gradients being reduced nor the parameters about to change.  The all-reduce of the other network's flat
    # gradient is a forked branch INSIDE graph A -- fork at the graph's root, join at its end -- so the collective node is off the critical
    # path of part A's kernels and there is no cross-stream event between replays (an event hop between a replay and another stream costs
    # 0.25-0.75 ms on this stack, scripts/cross_stream_cost.py).  Adam and the operand refresh stay eager on the main stream behind graph A
    # (lr_t is a by-value scalar; streaming kernels beside the persistent conv blocks cost the main stream 5 %, measured).
    def _apply_g_pending(self):
        """The generator's pending step (`_g_pending`: its lr_t) on the gradient in its flat buffer, already all-reduced."""
        lr_t, self._g_pending, self._g_pending_om = self._g_pending, None, None
        self._adam(self.g_params, lr_t, self.hyper_params.generator_beta1, self.hyper_params.generator_beta2)

    def _join_updates(self):
        """The one-graph and the pipelined iteration leave the generator's update pending, its gradient not yet all-reduced (the next
        iteration's graph does both): reduce and apply it here.  Data parallel: this IS a collective -- every rank must get here at the
        same point of its launch sequence.  train() therefore joins on EVERY rank before a rank-0 checkpoint and at its end;
        synchronize(), state_dict / checkpoint.save and generate() called by hand on a distributed model must be called on all ranks
        (`collective_pending()` tells whether the call would communicate)."""
        if self._g_pending is not None:
            self._reduce(self.g_params)
            self._apply_g_pending()

    def collective_pending(self):
        """True when the next _join_updates() / synchronize() / generate() / checkpoint would issue a gradient all-reduce."""
        return self.distributed and self.world > 1 and self._g_pending is not None

    def synchronize(self):
        """Everything a train_step enqueued (including the pending update) has finished.  Collective when `collective_pending()`."""
        self._join_updates()
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    def _overlap_in_graph(self):
        """The gradient all-reduce as a forked branch of the other run's part-A graph: data parallel, own RCCL communicator, in-graph
        collectives not refused (GS_NO_GRAPH_ALLREDUCE / a failed capture), not switched off (GS_NO_OVERLAP_REDUCE=1)."""
        return self._with_collective() and self.overlap_reduce

    def _pipelined_ok(self):
        return self._graphable() and self._overlap_in_graph()

    def _capture_pair(self, which, a_inputs, b_inputs, reduce_params):
        """Two graphs for one run: part A (own network) and part B (the rest), sharing one memory pool (replayed A, B, A, B ...).
        `reduce_params`: the OTHER network's parameters, whose flat gradient is all-reduced on a forked branch of graph A."""
        sa = [t.detach().clone() for t in a_inputs]
        sb = [t.detach().clone() for t in b_inputs]
        with self._capture_session(pipe=True):
            self._warm_up(lambda: self._part_b(which, self._part_a(which, *sa), *sb), reduce=[reduce_params], clear=[self._params_of(which)])
            ga = torch.cuda.CUDAGraph()
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                with self._capturing_into(ga, with_collective=True):
                    main = torch.cuda.current_stream()
                    fork = torch.cuda.Stream()
                    while fork.cuda_stream == main.cuda_stream or (self._side is not None and fork.cuda_stream == self._side.cuda_stream):
                        fork = torch.cuda.Stream()   # (pooled streams come round-robin: never the capturing one, nor the branches')
                    fork.wait_stream(main)            # fork at the root of the graph ...
                    with torch.cuda.stream(fork):
                        self._reduce_in_capture(reduce_params)
                    part_a = self._part_a(which, *sa)
                    main.wait_stream(fork)            # ... join at its end: the collective runs beside all of part A
            # Part A may hold NO kernel: a discriminator whose whole depth runs in the batched tail has no trunk of its own (shallow
            # growing regimes), and on ONE rank RCCL short-cuts the all-reduce to nothing as well.  torch warns about the empty graph;
            # that is the only way it can be empty -- with peers the collective is a node -- and an empty part A is simply not replayed.
            a_empty = any("Graph is empty" in str(w.message) for w in caught)
            for w in caught:
                if "Graph is empty" not in str(w.message):
                    warnings.warn_explicit(w.message, w.category, w.filename, w.lineno)
            if a_empty and self.world > 1:
                raise RuntimeError("part A of the %s run captured no node although it holds a gradient all-reduce over %d ranks" % (which, self.world))
            gb = torch.cuda.CUDAGraph()
            with self._capturing_into(gb, pool=ga.pool()):
                loss = self._part_b(which, part_a, *sb)
        return self._record(sa + sb, a=ga, b=gb, loss=loss, reduces=True, a_empty=a_empty)

    def _train_step_pipelined(self, d_latents, d_labels, real_images, g_latents, g_labels):
        """D.A | update G | D.B | G.A | update D | G.B (see above)."""
        hp = self.hyper_params
        P = self._pipe
        head, fade = self._regime()
        key = (head, fade is None, self.keep_gradients)
        self._set_fade(fade)
        d_in = ((d_labels, real_images), (d_latents, d_labels))   # (part A's inputs, part B's)
        g_in = ((g_latents, g_labels), (g_labels,))
        inputs = d_in[0] + d_in[1] + g_in[0] + g_in[1]
        if P is None or P["key"] != key or self._stale(P["d"], d_in[0] + d_in[1]) or self._stale(P["g"], g_in[0] + g_in[1]):
            self._join_updates()
            self._drop_captures(new_regime=P is not None and P["key"][:2] != key[:2])
            self._pipe = None
            P = self._capture_agreed(lambda: {"key": key, "d": self._capture_pair("d", *d_in, self.g_params),
                                              "g": self._capture_pair("g", *g_in, self.d_params)}, True, abandon=("d", "g"))
            if P is None:
                return self._plain_iteration(d_latents, d_labels, real_images, g_latents, g_labels)
            self._pipe = P
        D, G = P["d"], P["g"]
        _copy_inputs(D["static"] + G["static"], inputs)
        # D run.  Graph A = {D part A  ||  all-reduce of the generator's pending gradient}; then the generator's update (part B runs
        # the generator), then part B.
        self._arm(self.d_params)
        if not D["a_empty"]:
            D["a"].replay()
        if self._g_pending is not None:
            self._apply_g_pending()
        D["b"].replay()
        # G run.  Graph A = {G part A  ||  all-reduce of the discriminator's gradient}; the discriminator's update; part B runs it.
        self._arm(self.g_params)
        if not G["a_empty"]:
            G["a"].replay()
        self._apply(self.d_params, hp.discriminator_learning_rate, hp.discriminator_beta1, hp.discriminator_beta2, reduced=True)
        G["b"].replay()
        # the generator's step is left pending: its gradient is reduced inside the next D graph (or eagerly by _join_updates)
        self.g_params.t += 1
        self._g_pending = self._lr_t(hp.generator_learning_rate, hp.generator_beta1, hp.generator_beta2, self.g_params.t)
        self._g_pending_om = self._one_minus(self.g_params.t) if self._averaging() else None
        self.global_step += 1  # models.py:84
        self.discriminator_loss, self.generator_loss = D["loss"], G["loss"]
        return D["loss"], G["loss"]

    # ------------------------------------------------------------------- merged iteration
    # One GPU, graphs with branches: part A of the GENERATOR run (G(z) and the mode-seeking first-order pass: its own network only, whose
    # parameters the discriminator run does not touch) is captured INSIDE the discriminator run's graph, on a stream of its own --
    # the discriminator run's second half is one stream wide (the fake pass and the early weight gradients are done, the R1
    # double-backward, the real pass's backward and the final contraction remain), and the generator's few-block levels fill from it and
    # into it.  Two graphs per iteration:   X = { D run  ||  G.A }   update D   Y = { G.B }   update G.
    # 5.13 / 5.07 -> 4.99 / 4.93 ms on one box against one graph per run.
    # The generator's own-network nodes were created on that stream, so autograd runs their backward there in Y as well (joined at the
    # end of the run, _part_b).
    def _merged_ok(self):
        # (data parallel: with the gradient all-reduce as the last node of each of the two graphs -- own communicator, in-graph collectives
        #  not refused, not the four-graph overlapped form)
        dp_ok = not self.distributed or (self._with_collective() and not self._overlap_in_graph())
        return (self.merge_runs and self.fork and self._graphable() and dp_ok and self._fused_losses() and hasattr(kernels.get(), "lib"))

    # One graph per iteration (`fuse_iteration`, GS_NO_FUSED_ITERATION=1 returns to the pair above).  The two optimizer steps were the
    # only eager launches left between the graphs -- lr_t is a by-value scalar -- and with them outside, (i) every iteration pays two graph
    # boundaries, (ii) nothing can run beside an update, and (iii) data parallel, an all-reduce can only be the LAST node of a graph: exposed.
    # gs_adam_tf_step_dev reads lr_t from device memory, so the whole iteration is ONE graph Z:
    #     Z_k = { D real pass + R1 first-order pass        ||  [all-reduce G_{k-1}] -> Adam G_{k-1} -> refresh G -> D run's fake pass }
    #           -> D loss -> { D backward, contraction [all-reduce D_k] -> Adam D_k -> refresh D   ||  G.A_k }  ->  G.B_k
    # The GENERATOR's update of iteration k - 1 rides at the front of Z_k on the fake pass's branch: the discriminator's real pass and its R1
    # passes need nothing of the generator, and the fake pass (G fwd + D fwd + D bwd = 4 network passes against ~7 on the real side) has the
    # slack.  Data parallel this is where the generator's all-reduce hides by construction.  The discriminator's update sits where it always
    # did -- behind its backward -- but part A of the generator run is still in flight beside it.  After Z_k the generator's gradient is
    # PENDING (`_g_pending` holds its lr_t): the next replay applies it (lr slot >= 0), anything else that needs the weights -- generate(),
    # a checkpoint, a run outside this path, a new growing regime -- goes through _join_updates() first.  A freshly captured Z finds no
    # pending step: its lr slot is negative and the kernel leaves every buffer untouched.
    def _fused_ok(self):
        K = kernels.get()
        return self.fuse_iteration and hasattr(K, "adam_tf_step_dev") and (not self._averaging() or hasattr(K, "ema_step_dev"))

    def _apply_in_graph(self, params, slot, beta1, beta2, reduce_first=False):
        """The optimizer step as nodes of the graph being captured: [all-reduce] -> Adam with lr_t from the device table -> operand refresh.
        The generator's (slot 1) with an averaged generator: the average's update follows on the SAME stream, its 1 - decay_t in slot 2
        (negative with the step's lr_t: no step pending, no update) -- one node more on the fake pass's branch, no branch more (the graph
        already uses the runtime's four hardware queues).  Behind the refresh by default: DESIGN.md "Averaged generator"."""
        K = kernels.get()
        if reduce_first:
            self._reduce_in_capture(params)
        average = slot == 1 and self._averaging()
        early = average and self.ema_before_refresh
        K.adam_tf_step_dev(params.flat, params.grad, params.m, params.v, self._opt_scalars.ptr(slot), beta1, beta2, 1.0e-8,
                           1.0 / self.world, refresh=not early, zero_grad=not self.keep_gradients)
        if average:
            K.ema_step_dev(params.avg, params.flat, self._opt_scalars.ptr(2))
        if early:
            K.invalidate_weights(params.flat)
            K.refresh_weights(params.flat)

    def _capture_merged(self, d_inputs, g_inputs, fused=False):
        """The record of X and Y (`fused`: of Z, "y" is None), or None when the capture refused a collective on some rank."""
        K = kernels.get()
        hp = self.hyper_params
        sd = [t.detach().clone() for t in d_inputs]
        sg = [t.detach().clone() for t in g_inputs]
        both = (self.d_params, self.g_params)
        with_collective = self._with_collective()

        def d_run_beside_part_a_of_g():
            """The discriminator run (data parallel: ends with the all-reduce of its gradient, _part_b), `fused` with both optimizer
            steps; part A of the generator run forks off at its loss and is joined at the end.  Returns (d_loss, part A of the G run)."""
            main = torch.cuda.current_stream()
            side2 = self._second_stream("_side2", [main, self._side])
            box = []
            if fused:
                # the generator's PENDING step at the front of the fake pass's branch (no stream of its own: the branch is its only
                # consumer until the join, and a graph one branch wider would need one more of the runtime's four hardware queues)
                self._before_fake = lambda: self._apply_in_graph(self.g_params, 1, hp.generator_beta1, hp.generator_beta2,
                                                                 reduce_first=with_collective)

            def part_a_of_g():
                # from the discriminator run's loss on its second half is one stream wide (R1 double-backward, the real pass's backward,
                # the final contraction): part A of the generator run goes THERE (from the graph's root, beside the two forward passes,
                # measured 5.27 -> 5.34 ms)
                side2.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side2):
                    box.append(self._part_a("g", *sg))
                self.g_params.requires_grad_(False)      # (back to the discriminator run's arming for its backward)
                self.d_params.requires_grad_(True)
            self._after_loss = part_a_of_g
            d_loss = self._forward_backward("d", *sd)
            if fused:
                if self._before_fake is not None:
                    raise RuntimeError("the discriminator run never reached its fake pass: the generator's pending step has no place in the graph")
                # the discriminator's step, behind its (all-reduced) gradient; part A of the generator run is still in flight beside it
                self._apply_in_graph(self.d_params, 0, hp.discriminator_beta1, hp.discriminator_beta2)
            main.wait_stream(side2)
            return d_loss, box[0]

        def part_b_of_g(part_a):
            """Part B of the generator run (reads the discriminator just updated).  The generator's nodes will run on their stream again
            (autograd): it joins the capture HERE, at the root of part B, as a child of the capturing stream -- joining later through an
            event of the other branch (the discriminator's gradient arrives from there) made the two branches each other's parent and
            hip::Stream::EndCapture recursed until the stack ran out."""
            self.g_params.requires_grad_(True)           # (the discriminator run in between armed the other network)
            self.d_params.requires_grad_(False)
            self._side2.wait_stream(torch.cuda.current_stream())
            self._nodes_on_side2 = True
            return self._part_b("g", part_a, sg[1])

        def capture():
            gx = torch.cuda.CUDAGraph()
            with self._capturing_into(gx, with_collective=with_collective):
                d_loss, part_a = d_run_beside_part_a_of_g()
                reduced = [self._captured_reduce] * 2
                if fused:   # part B in the same graph
                    self._pipe_capture = True   # (no all-reduce at the end of THIS run: it opens the next graph, beside the real pass)
                    return dict(x=gx, y=None, d_loss=d_loss, g_loss=part_b_of_g(part_a), reduced=reduced)
            gy = torch.cuda.CUDAGraph()
            with self._capturing_into(gy, pool=gx.pool(), with_collective=with_collective):
                g_loss = part_b_of_g(part_a)
            reduced[1] = self._captured_reduce
            return dict(x=gx, y=gy, d_loss=d_loss, g_loss=g_loss, reduced=reduced)

        with self._capture_session():
            self._warm_up(lambda: (self._forward_backward("d", *sd), self._forward_backward("g", *sg)),
                          reduce=both if with_collective else (), clear=both)
            if fused:
                if self._opt_scalars is None:
                    self._opt_scalars = F.DeviceScalars(self.g_params.flat.device, 3 if self._averaging() else 2)
                # the per-network refresh launches read descriptor tables that are built (host -> device) on first use: not inside a capture
                for params in both:
                    K.invalidate_weights(params.flat)
                    K.refresh_weights(params.flat)
            graphs = self._capture_agreed(capture, with_collective, abandon=("d", "g"))
        return None if graphs is None else self._record(sd + sg, fused=fused, **graphs)

    def _train_step_merged(self, d_latents, d_labels, real_images, g_latents, g_labels):
        hp = self.hyper_params
        head, fade = self._regime()
        fused = self._fused_ok()
        key = (head, fade is None, self.keep_gradients, fused)
        if not (fused and self._merged is not None and self._merged["key"] == key):
            self._join_updates()   # (the one-graph iteration applies a pending generator step itself, at the front of the replay)
        self._set_fade(fade)
        inputs = (d_latents, d_labels, real_images, g_latents, g_labels)
        M = self._merged
        if M is None or M["key"] != key or self._stale(M, inputs):
            self._join_updates()   # (a pending generator step belongs to the graph being dropped)
            self._drop_captures(new_regime=M is not None and M["key"][:2] != key[:2])
            self._merged = None
            M = self._capture_merged(inputs[:3], inputs[3:], fused=fused)
            if M is None:
                return self._plain_iteration(*inputs)
            M["key"] = key
            self._merged = M
        _copy_inputs(M["static"], inputs)
        if M["fused"]:
            self.d_params.t += 1
            self.g_params.t += 1
            lr_d = self._lr_t(hp.discriminator_learning_rate, hp.discriminator_beta1, hp.discriminator_beta2, self.d_params.t)
            scalars = [lr_d, -1.0 if self._g_pending is None else self._g_pending]
            if self._averaging():   # (the average follows the pending step, or nothing)
                scalars.append(-1.0 if self._g_pending is None else self._g_pending_om)
            self._opt_scalars.set(scalars)   # (stream-ordered before the replay)
            self._arm(self.d_params)
            if self._g_pending is None:
                self._arm(self.g_params)      # (no step at the front of this replay: the buffer must already be clean)
            self._g_pending = self._g_pending_om = None
            M["x"].replay()
            self.d_params.grad_clean = not self.keep_gradients
            self.g_params.grad_clean = False   # (holds the gradient of the step that is now pending)
            self._g_pending = self._lr_t(hp.generator_learning_rate, hp.generator_beta1, hp.generator_beta2, self.g_params.t)
            self._g_pending_om = self._one_minus(self.g_params.t) if self._averaging() else None
        else:
            self._arm(self.d_params)
            M["x"].replay()
            self._apply(self.d_params, hp.discriminator_learning_rate, hp.discriminator_beta1, hp.discriminator_beta2, reduced=M["reduced"][0])
            self._arm(self.g_params)
            M["y"].replay()
            self._apply(self.g_params, hp.generator_learning_rate, hp.generator_beta1, hp.generator_beta2, reduced=M["reduced"][1])
        self.global_step += 1  # models.py:84
        self.discriminator_loss, self.generator_loss = M["d_loss"], M["g_loss"]
        return M["d_loss"], M["g_loss"]
