"""How a run of the trainer is captured into a hipGraph and replayed -- once, for the three iteration forms of iteration.py.

A capture is: `_capture_session` (the fade-weight table installed on the networks, the per-capture hooks and flags reset when it ends or
raises) around one `_warm_up` and one or more `_capturing_into` blocks; what it leaves is one `_record`.  A replay is: `_stale` (capture
again?), `_copy_inputs` into the record's static tensors, `_arm` for every gradient buffer the graph accumulates into, `graph.replay()`.
`Capture` is a mix-in of models.GANSynth: the captured passes, the streams and the hooks are the trainer's own."""
import contextlib

import torch

from . import config
from . import fork_probe
from . import functional as F
from . import kernels

LEVEL_STREAMS = int(config.value("GS_LEVEL_STREAMS", "128"))   # see Capture._leveled_queues


def _capture_mode(with_collective, forked=False):
    """Keyword arguments of torch.cuda.graph for a capture that contains an RCCL collective: the communicator's helper threads may call
    the HIP runtime while this thread captures (proxy progress, registration), which the default "global" capture mode turns into a capture
    error on THEIR call -- captures with a collective inside run "thread_local" (only this thread's calls are checked), as captured NCCL
    work is run elsewhere.  With forked branches in the same capture (GANSynth._branch: autograd's device thread then records and waits on
    events between two captured streams) a thread_local capture replayed into a segmentation fault on this stack (ROCm 7.0.2, RCCL 2.26.6,
    one rank; "global" and "relaxed" captures of the same run replay fine): those captures are "relaxed" (no thread's calls are checked).
    Everything else keeps the strict default."""
    forced = config.value("GS_CAPTURE_MODE")   # (debugging)
    if forced:
        return {"capture_error_mode": forced}
    if not with_collective:
        return {}
    return {"capture_error_mode": "relaxed" if forked else "thread_local"}


def _copy_inputs(dsts, srcs):
    """A run's inputs into the static buffers its graph reads: ONE multi-tensor launch where the tensors allow it (same device, dtype and
    strides pairwise) instead of a ~5 us copy kernel per input in front of every replay."""
    dsts, srcs = list(dsts), list(srcs)
    pairs = [(d, s) for d, s in zip(dsts, srcs) if d.data_ptr() != s.data_ptr()]
    if not pairs:
        return
    # (only the SMALL inputs share a launch: the multi-tensor kernel moves a 4 MB image batch on 34 blocks -- 21 us against 5 for its own copy)
    small = [(d, s) for d, s in pairs if d.numel() * d.element_size() <= (256 << 10)]
    if len(small) > 1 and all(d.is_cuda and s.is_cuda and d.dtype == s.dtype == small[0][0].dtype and d.stride() == s.stride() for d, s in small):
        torch._foreach_copy_([d for d, _ in small], [s for _, s in small])
        pairs = [(d, s) for d, s in pairs if d.numel() * d.element_size() > (256 << 10)]
    for d, s in pairs:
        d.copy_(s)


@contextlib.contextmanager
def _quiet_gc():
    """Collect garbage NOW and keep the cyclic collector off while a hipGraph is being captured: a collection in the middle of a
    capture may destroy an old CUDAGraph / event of an earlier trainer (a destructor that is illegal during capture: the process
    aborts).  torch.cuda.graph no longer collects on entry by itself."""
    import gc
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class Capture(object):

    @contextlib.contextmanager
    def _leveled_queues(self):
        """Around a capture whose graph may hold parallel branches: LEVEL_STREAMS throw-away streams exist while the graph is instantiated
        (torch does that when the capture ends), so that the streams the HIP runtime makes for the branches land on different hardware
        queues -- see gs_streams_create in include/gansynth_hip.h for the runtime defect this keeps hipGraphLaunch away from."""
        # (also without branches of our own: the data-parallel graphs fork for their all-reduce)
        K = kernels.get() if ((self.fork or self.distributed) and torch.cuda.is_available()) else None
        if K is None or not hasattr(K, "lib") or LEVEL_STREAMS <= 0:
            yield
            return
        import ctypes
        from . import _lib
        handles = (ctypes.c_void_p * LEVEL_STREAMS)()
        ptr = ctypes.cast(handles, ctypes.POINTER(ctypes.c_void_p))
        t0 = __import__("time").perf_counter()
        try:
            _lib.check(K.lib.gs_streams_create(LEVEL_STREAMS, ptr), "gs_streams_create")   # (on failure the ones made so far are in `handles`)
            self.level_seconds = getattr(self, "level_seconds", 0.0) + __import__("time").perf_counter() - t0
            yield
        finally:
            _lib.check(K.lib.gs_streams_destroy(LEVEL_STREAMS, ptr), "gs_streams_destroy")

    def _check_fork_runtime(self):
        """Before the first capture that may hold parallel branches (see fork_probe._forked_replay_ok)."""
        if self.fork and torch.cuda.is_available() and not fork_probe._forked_replay_ok():
            self.fork = False

    def _second_stream(self, which, avoid):
        """A pooled stream for a branch that is none of `avoid` (torch.cuda.Stream() hands out 32 pooled streams round-robin: after enough
        captures -- every one takes a warm-up stream -- the next one IS the stream being captured: a branch that waits for itself)."""
        cur = getattr(self, which)
        taken = {a.cuda_stream for a in avoid if a is not None}
        if cur is None or cur.device != avoid[0].device or cur.cuda_stream in taken:
            for _ in range(64):
                cur = torch.cuda.Stream(device=avoid[0].device)
                if cur.cuda_stream not in taken:
                    break
            else:
                raise RuntimeError("no further stream for the forked branches of a captured run")
            setattr(self, which, cur)
        return cur

    def _stream_guard(self):
        K = kernels.get()
        if self.fork and hasattr(K, "stream_guard") and torch.cuda.is_available():
            return K.stream_guard()
        return contextlib.nullcontext()

    @staticmethod
    def _capturing():
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

    # ------------------------------------------------------------------------ one capture
    @contextlib.contextmanager
    def _capture_session(self, pipe=False):
        """Around the warm-up and the captures of one record.  The networks read the fade weight from the device table for its duration (eager
        callers keep passing the number).  `pipe`: the caller places the gradient all-reduces itself, none at the end of part B.  Every hook and
        flag a capture arms is cleared HERE, also when it raises: a failed capture must not leave a hook armed for an unrelated run."""
        owner = getattr(self.generator, "__self__", None)
        _, fade = self._regime()
        owner.fade_weight = self._lerp if fade is not None else None
        self._pipe_capture = pipe
        try:
            yield
        finally:
            owner.fade_weight = None
            self._after_loss = self._before_fake = None
            self._nodes_on_side2 = self._pipe_capture = self._warming_up = False

    def _warm_up(self, run, reduce=(), clear=()):
        """Before a capture: `run()` once eagerly on a side stream (allocator / lazy-init warm-up), then one eager all-reduce of every
        parameter set in `reduce` -- RCCL sets up its channels on the first collective of a kind, which is not capturable; every rank does
        the same and the gradients are dead values here."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        self._warming_up = True
        try:
            with torch.cuda.stream(side):
                run()
                for params in reduce:
                    self._reduce(params)
        finally:
            self._warming_up = False
        torch.cuda.current_stream().wait_stream(side)
        # the warm-up pass left its gradients in the flat buffers and no optimizer step clears them: a graph that relies on the step's
        # clearing (keep_gradients = False: no fill inside) must find the buffer as every later replay will
        if not self.keep_gradients:
            for params in clear:
                params.grad.zero_()
                params.grad_clean = True
        # the prepared weight operands live in persistent workspaces that the optimizer step refreshes eagerly (kernels.adam_tf_step):
        # bring them up to date now so that the captured graph holds no re-layout launches
        kernels.get().refresh_weights()

    @contextlib.contextmanager
    def _capturing_into(self, graph, pool=None, with_collective=False):
        """`with self._capturing_into(graph):` -- the launches inside become the nodes of `graph`."""
        self._captured_reduce = False   # (set by _part_b when the run's all-reduce went into the graph)
        with _quiet_gc(), self._leveled_queues(), self._stream_guard(), torch.cuda.graph(graph, pool=pool, **_capture_mode(with_collective, self.fork)):
            yield

    def _capture_agreed(self, capture, with_collective, abandon):
        """`capture()`, or None when the collective would not go into a graph on SOME rank.  A capture with a collective inside may fail
        on one rank alone; its outcome is agreed on (_agree), so that no rank keeps a graph with the collective inside while a peer
        reduces eagerly, and on "no" EVERY rank drops the in-graph form and the state the failed capture of the runs in `abandon` left:
        from then on the all-reduce follows each replay eagerly (_run).  Without a collective inside an error is just raised."""
        error, out = None, None
        try:
            out = capture()
        except RuntimeError as e:
            if not with_collective:
                raise
            error = e
        if with_collective and not self._agree(error is None):
            self._give_up_graph_collectives(abandon[0], error)
            for which in abandon[1:]:
                self._abandon_capture(which)
            return None
        return out

    def _record(self, static, **fields):
        """What a capture is stored as: what its form names in `fields` (graphs, losses), the static tensors the graphs read their inputs from,
        whether they were captured to keep gradients (else: no fill inside, they rely on the zeroing optimizer step behind every replay), and
        the cached junction constants they read (alive as long as the graphs)."""
        return dict(fields, static=static, keep=self.keep_gradients, consts=F.constants_snapshot())

    # ------------------------------------------------------------------------ one replay
    def _stale(self, record, inputs):
        return (record is None or record["keep"] != self.keep_gradients
                or any(a.shape != b.shape or a.dtype != b.dtype for a, b in zip(record["static"], inputs)))

    def _drop_captures(self, new_regime):
        """Before capturing again.  A new growing regime has other junction constants (live graphs hold their own references to the old ones)."""
        self._graphs.clear()
        if new_regime:
            F.drop_constants()

    def _set_fade(self, fade):
        """The one per-step scalar of a captured run, the fade-in weight, is read from device memory: stream-ordered before the replay."""
        if fade is not None:
            if self._lerp is None:
                self._lerp = F.DeviceLerp(self.g_params.flat.device)
            self._lerp.set(fade)

    def _arm(self, params):
        """A no-fill graph is about to accumulate into this buffer, as begin_run did at capture time: it must be clean -- it is behind the
        zeroing update of the last replay, it is not e.g. when a run is repeated without its optimizer step."""
        if not self.keep_gradients:
            if not params.grad_clean:
                params.grad.zero_()
            params.grad_clean = False

    def _abandon_capture(self, which):
        """State left behind by a _forward_backward that raised in the middle of a stream capture: deferred kernel-layer jobs, half-built
        fusion hand-offs and the gradients the partial backward wrote."""
        torch.cuda.synchronize()
        K = kernels.get()
        if hasattr(K, "drop_deferred"):
            K.drop_deferred()
        F.reset_fusion_state()
        self._inflight = None
        self._marks.clear()
        params = self.d_params if which == "d" else self.g_params
        if not self.keep_gradients:   # (as before the first capture: a graph without a fill must find the buffer the way every replay will)
            params.grad.zero_()
            params.grad_clean = True
