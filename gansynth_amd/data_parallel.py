"""Data parallelism of the trainer (new -- the reference is single GPU): the gradient all-reduce and the votes that keep every rank on
the same launch sequence.  A mix-in of models.GANSynth: it reads the trainer's parameters, communicator and capture state."""
import torch

from . import config
from . import kernels


class DataParallel(object):

    # Data parallelism (the reference is single-GPU): the flat gradient of a network is all-reduced in BUCKETS of
    # whole tensors (<= bucket_bytes; the generator's 16.8 MB dense weight alone), in the order the backward pass completes them,
    # and the TF-Adam update runs bucket by bucket behind its all-reduce; in eager mode the first buckets are launched from inside
    # the backward's tail (the per-layer weight-gradient contraction, kernels.flush_wgrad_reductions) as soon as their last
    # gradient is written.  The 1/world averaging is folded into the Adam kernel.
    # Two transports.  (i) Default on HIP: libgansynth_hip.so's own RCCL communicator (comm.py, gs_comm_*), every collective on
    # the backward's stream.  Nothing overlaps then -- and nothing needs an event: measured on one MI355X (RCCL, world 1, graphs):
    # 7.31 ms per iteration against 7.28 without any collective, whereas two all-reduces through torch.distributed's
    # communicator stream cost 0.43-0.49 ms of cross-stream hops (7.71-7.82 ms) before a single byte moves.  One bucket per network
    # by default (fewest launches).  (ii) torch.distributed's collectives (CPU / gloo tests, GS_TORCH_COLLECTIVES=1): asynchronous
    # on the communicator's stream, bucket k+1 on the wire under the update of bucket k.
    def _launch_reduce(self, params, bucket):
        a, b = params.buckets[bucket]
        if self._comm is not None:   # same stream as the backward: ordered by the stream itself, no event hop
            return self._comm.all_reduce_(params.grad[a:b])
        return torch.distributed.all_reduce(params.grad[a:b], async_op=True)

    def _reduce(self, params):
        """Blocking form (pipelined step): every bucket reduced, in order, on the current stream's timeline."""
        if self.distributed:
            for i in range(len(params.buckets)):
                self._launch_reduce(params, i).wait()

    def _apply(self, params, lr, beta1, beta2, reduced=False):
        params.t += 1
        lr_t = self._lr_t(lr, beta1, beta2, params.t)
        if not self.distributed or reduced:
            self._adam(params, lr_t, beta1, beta2)
            return
        K = kernels.get()
        zero = not self.keep_gradients
        works = {}
        if self._inflight is not None and self._inflight[0] is params:
            works = dict(self._inflight[1])
        self._inflight = None
        for i in range(len(params.buckets)):
            if i not in works:
                works[i] = self._launch_reduce(params, i)
        for i, (a, b) in enumerate(params.buckets):
            works[i].wait()   # (stream-side wait: the host does not block)
            K.adam_tf_step(params.flat[a:b], params.grad[a:b], params.m[a:b], params.v[a:b], lr_t, beta1, beta2, 1.0e-8,
                           1.0 / self.world, refresh=False, zero_grad=zero)
        params.grad_clean = zero   # (the buckets cover the whole buffer)
        K.invalidate_weights(params.flat)
        K.refresh_weights(params.flat)
        # the averaged generator: ONE launch over the whole buffer behind the last bucket, not one per bucket.  The average is a function of
        # the weights alone, and those are identical on every rank after the all-reduce: so is the average, with no communication.
        self._average_after(params)

    def _arm_first_bucket(self, K, params):
        """Data parallel, captured discriminator run, OPT-IN (`bucket_d_reduce`, GS_DP_BUCKET_D=1): the all-reduce of the gradient in two steps.
        (Opt-in because of what it measured, DESIGN.md 7: with 300-us stand-ins for the collectives -0.09 ... -0.14 ms fully grown, +0.15 ms in a
        fade-in regime, +0.03 with 150-us ones.)
        The layers with >= 128 input channels (and the one-channel slice of the last block's conv) hold ~90 % of the bytes and sit at the BOTTOM of
        the pyramid: every pass of the backward is done with them long before it ends.  kernels.complete_rule tells when the last of their pairs
        is recorded; their contraction then runs on the branch (as the early contraction of the large layers does), and behind it, on the branch
        as well, the all-reduce of the largest range of the flat buffer that holds none of the OTHER layers' gradients -- beside the rest of the
        backward and the final contraction.  What is left on either side of that range follows where the one message went."""
        self._split_at, self._first_bucket_stream = None, None
        if not (self.bucket_d_reduce and self.distributed and self._comm is not None and self._graph_allreduce and self._capturing()
                and not self._pipe_capture and hasattr(K, "complete_rule")):
            return
        pred = lambda key: int(key[5][0]) >= 128 or int(key[5][0]) == 1   # (key: kernels._defer_wgrad; [5] = the conv input's (channels, h, w))
        named = list(params.named.items())
        sibling = {}   # weight gradient -> its bias gradient (a layer's bias follows its weight; it is complete when the layer is)
        for (name, p), (name2, p2) in zip(named, named[1:]):
            if name.endswith("/weight") and name2 == name[:-len("weight")] + "bias":
                sibling[p.grad.data_ptr()] = p2.grad
        base, size, total = params.grad.data_ptr(), params.grad.element_size(), params.grad.numel()

        def on_complete(select, others):
            def then():
                K.flush_bias_folds()
                spans = []
                for out, bias in others:
                    for t in (out, bias, sibling.get(out.data_ptr())):
                        if t is not None:
                            a, b = K._span(t)
                            spans.append(((a - base) // size, (b - base + size - 1) // size))
                if any(not (0 <= a < b <= total) for a, b in spans):
                    return   # (a gradient outside the flat buffer: the one message at the end)
                edges, at = [], 0
                for a, b in sorted(spans):
                    edges.append((at, max(at, a)))
                    at = max(at, b)
                edges.append((at, total))
                first = max(edges, key=lambda e: e[1] - e[0])
                if first[1] - first[0] > 0:
                    self._split_at = self.first_bucket = first
                    if config.flag("GS_DEBUG_DP_BUCKET"):
                        print("first bucket", first, "of", total, "behind", sum(1 for _ in others), "other layers", flush=True)
                    # on a stream of its own, behind the contraction just issued: the branch goes on to the final contraction's thin layers, and
                    # nothing of this run waits for the message before the messages at the end do (_part_b)
                    done = torch.cuda.Event()
                    done.record()
                    cur = torch.cuda.current_stream()
                    third = self._second_stream("_side3", [cur, self._origin, self._side, self._side2])
                    third.wait_event(done)
                    with torch.cuda.stream(third):
                        self._comm.all_reduce_(params.grad[first[0]:first[1]], marker_share=(first[1] - first[0]) / total)
                    self._first_bucket_stream = third
            self._early_flush(select, then=then)
        K.complete_rule(pred, on_complete)

    def _reduce_in_capture(self, params):
        """The gradient all-reduce issued while the current stream is being captured into a hipGraph (a method of its own so that a
        test can make it raise and watch every rank fall back together)."""
        self._reduce(params)

    def _agree(self, ok):
        """Data parallel: did EVERY rank succeed?  A rank-local failure (allocator, capture) must not leave one rank on a different
        launch sequence than its peers -- their collectives would no longer pair up and the job would hang -- so the outcome of
        anything that may fail locally is agreed on with an eager MIN all-reduce over the launcher's process group, outside any
        capture, and every rank takes the same branch."""
        if not self.distributed or self.world <= 1:
            return bool(ok)
        return self._vote(ok, self.g_params.flat.device)

    @staticmethod
    def _vote(ok, device):
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=device)
        torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
        return bool(flag.item())

    def _give_up_graph_collectives(self, which, error):
        """Every rank lands here together (see _agree): no collective inside captured graphs any more.  A capture that aborted with an
        ncclAllReduce inside may have left our communicator unusable, so the eager collectives move to torch.distributed's own."""
        import sys
        print("gansynth_amd.models: capturing the gradient all-reduce inside the %s run's graph failed on some rank (here: %s); "
              "it will run eagerly after each replay" % (which, "ok" if error is None else str(error).splitlines()[0]), file=sys.stderr, flush=True)
        self._graph_allreduce = False
        # Every graph captured so far may replay an ncclAllReduce on the communicator given up here (the OTHER run's graph of the
        # serial path, the pairs of the pipelined step): all of them go, so that every run is captured again without a collective.
        torch.cuda.synchronize()
        self._graphs.clear()
        self._merged = None
        self._pipe = None
        if self.world > 1 and self._comm is not None:
            # Not destroyed: ncclCommDestroy on a communicator an aborted capture left half-enqueued may block.  It is retired --
            # never used again, kept alive until the process ends -- and the eager collectives go through torch.distributed.
            self._retired_comm = self._comm
            self._comm = None
        self._abandon_capture(which)

    def _all_ranks_have_input(self, have):
        """Data parallel: the input shards are rank-local (files[rank::world], per-record filters), so they run dry at different
        steps; a rank that stopped alone would leave the others blocked in the next all-reduce.  Every rank votes before each
        iteration and all stop together at the first "no" (the reference's single process stops at its OutOfRangeError,
        models.py:193).  Inputs that cannot run dry (`real_input_fn.finite == False`) skip the vote and its host sync."""
        if not self.distributed or not getattr(self.real_input_fn, "finite", True):
            return have
        dev = self.g_params.flat.device if self.g_params is not None else (torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"))
        return self._vote(have, dev)
