"""Differentiable (to second order) wrappers around the HIP kernels.

The reference obtains its R1 penalty and mode-seeking loss from nested tf.gradients
(models.py:47,60), i.e. it differentiates through the backward pass.  Each op here is a
torch.autograd.Function whose backward is itself expressed with Functions, so
`torch.autograd.grad(..., create_graph=True)` composes exactly like tf.gradients does:

  conv / conv-transpose / dense : the three bilinear maps (fwd, bwd-data, bwd-weight) are closed
                                  under differentiation -- each one's gradients are the other two;
  bias+activation, pixel-norm, tanh, batch-stddev : explicit first- and second-order kernels;
  upscale / block-sum : adjoint pair.

torch is only the tape; every tensor operation is a kernel from libgansynth_hip.so.
"""
import contextlib
import itertools

import torch
from torch.autograd.function import once_differentiable

# The autograd engine runs the READY node with the highest sequence number first, and torch numbers nodes from THREAD-LOCAL counters: the nodes of
# a second-order graph are created on the engine's device thread (inside Function.backward bodies, under create_graph), everything else on the
# caller's thread, so which of two independent ready nodes runs first depended on how far each thread's counter had got -- on what the process
# did before.  The launches of a run were the same set either way, but gradients with several contributions (a dense weight fed by the real
# pass, the fake pass and the R1 term) were summed in another ORDER: last-bit differences that TF-Adam's sign-like first steps turn into 2 lr on
# the elements whose gradient is round-off sized (seen: the same test green inside the suite and 8e-4 apart in a fresh process).  Every Function of
# this module therefore numbers its node from ONE process-wide counter, far above anything a thread-local counter reaches: among the nodes of this
# library the engine's order is the reverse of their creation order, whatever thread created them and whatever ran before.
_NODE_SEQ = itertools.count(1 << 40)


def _number_node(out):
    t = out[0] if isinstance(out, (tuple, list)) and out else out
    fn = getattr(t, "grad_fn", None) if isinstance(t, torch.Tensor) else None
    if fn is not None and hasattr(fn, "_set_sequence_nr"):
        fn._set_sequence_nr(next(_NODE_SEQ))


class Function(torch.autograd.Function):
    """torch.autograd.Function whose nodes take their engine priority from the process-wide counter above."""

    @classmethod
    def apply(cls, *args, **kwargs):
        out = super().apply(*args, **kwargs)
        _number_node(out)
        return out


from . import config
from . import kernels
from ._lib import ACT_LRELU, ACT_NONE, ACT_TANH


def _K():
    return kernels.get()


# ---- activation tap ---------------------------------------------------------------------------------------------------------
# Parity tests compare this path with the oracle on the SAME linear pieces of leaky_relu (a pre-activation within an fp32 ulp
# of 0 may fall on either side, which moves that unit's gradient 5x -- tests/test_model_gpu.py).  Inside `activation_tap()`
# every forward network call records (name, [leaky_relu outputs in call order]); nothing else changes.
class activation_tap(object):
    active = None

    def __init__(self):
        self.calls = []
        self.pair = None   # (call index of the real pass, of the fake pass) while one launch serves both (tap_pair)

    def __enter__(self):
        activation_tap.active = self
        return self

    def __exit__(self, *exc):
        activation_tap.active = None
        return False

    def masks(self):
        """[(network name, [z > 0 as CPU bool tensors, logical layout])] -- what oracle.torch_ref.lrelu_tape("override") takes."""
        return [(name, [(z > 0).cpu().contiguous() for z in zs]) for name, zs in self.calls]


def tap_begin(name):
    if activation_tap.active is not None:
        activation_tap.active.calls.append((name, []))


def tap_index():
    """Index of the network call being recorded (None outside a tap)."""
    return None if activation_tap.active is None else len(activation_tap.active.calls) - 1


class tap_pair(object):
    """While active, a recorded activation holds two batches (axis 0): its halves go to the calls `a` and `b` -- the discriminator's tail
    run once over [real; fake] (models.GANSynth._d_losses_b_batched) still reads as the reference's two passes."""

    def __init__(self, a, b):
        self.pair = None if a is None or b is None else (a, b)

    def __enter__(self):
        if activation_tap.active is not None:
            activation_tap.active.pair = self.pair
        return self

    def __exit__(self, *exc):
        if activation_tap.active is not None:
            activation_tap.active.pair = None
        return False


def _tap(z, act):
    tap = activation_tap.active
    if tap is not None and act == ACT_LRELU:
        if tap.pair is not None:
            n = z.shape[0] // 2
            tap.calls[tap.pair[0]][1].append(z[:n].detach())
            tap.calls[tap.pair[1]][1].append(z[n:].detach())
        else:
            tap.calls[-1][1].append(z.detach())


# ------------------------------------------------------------------ bilinear map families
class _ConvKind(object):
    """tf.nn.conv2d SAME (ops.py:237-243), ksize in {1,3}, stride in {1,2}."""

    def __init__(self, ksize, stride):
        self.ksize, self.stride = ksize, stride

    def fwd(self, x, w, alpha):
        return _K().conv2d_fwd(x, w, self.ksize, self.stride, alpha)

    def fwd_bias_act(self, x, w, bias, alpha, act):
        return _K().conv2d_fwd_bias_act(x, w, bias, self.ksize, self.stride, alpha, act)

    def fwd_mask(self, x, w, alpha, mask, mask_act):
        K = _K()
        if hasattr(K, "conv2d_fwd_mask"):
            return K.conv2d_fwd_mask(x, w, self.ksize, self.stride, alpha, mask, mask_act)
        return K.act_bwd(self.fwd(x, w, alpha), mask, mask_act)

    def fwd_bias_act_norm(self, x, w, bias, alpha, act, eps, want_z):
        K = _K()
        if hasattr(K, "conv2d_fwd_bias_act_norm"):   # (z, y) from one call; the norm rides in the conv epilogue where it can
            return K.conv2d_fwd_bias_act_norm(x, w, bias, self.ksize, self.stride, alpha, act, eps, want_z=want_z)
        z = self.fwd_bias_act(x, w, bias, alpha, act)
        return z, K.pixel_norm_fwd(z, eps)

    def bwd_data(self, gy, w, x_shape, alpha):
        return _K().conv2d_bwd_data(gy, w, x_shape, self.ksize, self.stride, alpha)

    def bwd_data_mask(self, gy, w, x_shape, alpha, mask, mask_act):
        return _K().conv2d_bwd_data(gy, w, x_shape, self.ksize, self.stride, alpha, mask=mask, mask_act=mask_act)

    def bwd_data_pnbwd(self, gy, w, x_shape, alpha, z, eps, act, addend):
        return _K().conv2d_bwd_data_pnbwd(gy, w, x_shape, self.ksize, self.stride, alpha, z, eps, act, addend=addend)

    def bwd_data_pnbwd_is_fused(self, x_shape, co, dtype):
        K = _K()
        return hasattr(K, "bwd_data_pnbwd_is_fused") and K.bwd_data_pnbwd_is_fused(x_shape, co, self.ksize, self.stride, False, dtype)

    def fwd_pnbwdbwd(self, x, w, alpha, g, z, eps, act):
        return _K().conv2d_fwd_pnbwdbwd(x, w, self.ksize, self.stride, alpha, g, z, eps, act)

    def fwd_pnbwdbwd_is_fused(self, x_shape, co, dtype):
        K = _K()
        return hasattr(K, "fwd_pnbwdbwd_is_fused") and K.fwd_pnbwdbwd_is_fused(x_shape, co, self.ksize, self.stride, False, dtype)

    bias_in_wgrad = True   # the weight-gradient kernels can return the bias gradient of the block on the side

    def bwd_weight(self, x, gy, alpha, out=None, bias_out=None):
        return _K().conv2d_bwd_weight(x, gy, self.ksize, self.stride, alpha, out=out, bias_out=bias_out)


class _ConvTransposeKind(object):
    """tf.nn.conv2d_transpose 3x3 stride 2 SAME (ops.py:266-276)."""

    def fwd(self, x, w, alpha):
        return _K().conv2d_transpose_fwd(x, w, alpha)

    def fwd_bias_act(self, x, w, bias, alpha, act):
        return _K().conv2d_transpose_fwd_bias_act(x, w, bias, alpha, act)

    def fwd_bias_act_norm(self, x, w, bias, alpha, act, eps, want_z):
        K = _K()
        if hasattr(K, "conv2d_transpose_fwd_bias_act_norm"):
            return K.conv2d_transpose_fwd_bias_act_norm(x, w, bias, alpha, act, eps, want_z=want_z)
        z = self.fwd_bias_act(x, w, bias, alpha, act)
        return z, K.pixel_norm_fwd(z, eps)

    def bwd_data(self, gy, w, x_shape, alpha):
        return _K().conv2d_transpose_bwd_data(gy, w, alpha)

    def bwd_data_pnbwd(self, gy, w, x_shape, alpha, z, eps, act, addend):
        return _K().conv2d_transpose_bwd_data_pnbwd(gy, w, alpha, z, eps, act, addend=addend)

    def bwd_data_pnbwd_is_fused(self, x_shape, co, dtype):
        K = _K()
        return hasattr(K, "bwd_data_pnbwd_is_fused") and K.bwd_data_pnbwd_is_fused(x_shape, co, 3, 2, True, dtype)

    def fwd_pnbwdbwd(self, x, w, alpha, g, z, eps, act):
        return _K().conv2d_transpose_fwd_pnbwdbwd(x, w, alpha, g, z, eps, act)

    def fwd_pnbwdbwd_is_fused(self, x_shape, co, dtype):
        K = _K()
        return hasattr(K, "fwd_pnbwdbwd_is_fused") and K.fwd_pnbwdbwd_is_fused(x_shape, co, 3, 2, True, dtype)

    def bwd_weight(self, x, gy, alpha, out=None):
        return _K().conv2d_transpose_bwd_weight(x, gy, alpha, out=out)


class _DenseKind(object):
    """tf.matmul (ops.py:197)."""

    def fwd(self, x, w, alpha):
        return _K().dense_fwd(x, w, alpha)

    def fwd_bias_act(self, x, w, bias, alpha, act):
        if hasattr(_K(), "dense_fwd_bias_act"):
            return _K().dense_fwd_bias_act(x, w, bias, alpha, act)
        return _K().bias_act_fwd(_K().dense_fwd(x, w, alpha), bias, act)

    def bwd_data(self, gy, w, x_shape, alpha):
        return _K().dense_bwd_data(gy, w, alpha)

    def bwd_weight(self, x, gy, alpha, out=None):
        return _K().dense_bwd_weight(x, gy, alpha, out=out)


class _DenseFlatKind(object):
    """tf.matmul on tf.layers.flatten(x) of an NCHW activation (networks.py:185-186) with x kept in channels-last memory: the three
    maps take / return the 4-D activation, the flatten is a row map inside the kernels (a GsDense with c, hw set)."""

    def fwd(self, x, w, alpha):
        return _K().dense_fwd_nhwc(x, w, alpha)

    def fwd_bias_act(self, x, w, bias, alpha, act):
        if hasattr(_K(), "dense_fwd_bias_act"):
            return _K().dense_fwd_bias_act(x, w, bias, alpha, act)
        return _K().bias_act_fwd(_K().dense_fwd_nhwc(x, w, alpha), bias, act)

    def bwd_data(self, gy, w, x_shape, alpha):
        return _K().dense_bwd_data_nhwc(gy, w, x_shape, alpha)

    def bwd_weight(self, x, gy, alpha, out=None):
        return _K().dense_bwd_weight_nhwc(x, gy, alpha, out=out)


# ---- gradients w.r.t. data only -------------------------------------------------------------------------------------------
# tf.gradients(ys, xs) (models.py:47,60: the R1 penalty differentiates w.r.t. the real images, the mode-seeking term w.r.t. the
# latents) only builds what xs needs.  torch.autograd.grad(..., inputs) prunes nodes, but inside a node a custom Function is
# still asked for every input that requires grad -- i.e. the weight and bias gradients of every conv on the path, computed and
# thrown away (a quarter of all weight-gradient launches of an iteration).  The model wraps those two calls in this context.
_PARAM_GRADS = [True]


class data_grads_only(object):
    def __enter__(self):
        _PARAM_GRADS.append(False)

    def __exit__(self, *exc):
        _PARAM_GRADS.pop()
        return False


# A backward pass whose only clients are the parameters (the trainer's loss.backward(): tf.gradients(loss, var_list), models.py:67-89) has no
# use for the gradient of a LEAF activation -- the real image batch, which requires grad for the R1 term's own pass: the colour block's data
# gradient (67 MB read at 128x1024) is skipped there.
_PARAMS_ONLY = False


class params_only(object):
    def __enter__(self):
        global _PARAMS_ONLY
        self.was, _PARAMS_ONLY = _PARAMS_ONLY, not config.flag("GS_NO_PARAMS_ONLY")
        return self

    def __exit__(self, *exc):
        global _PARAMS_ONLY
        _PARAMS_ONLY = self.was
        return False


def _want_params():
    return _PARAM_GRADS[-1]


def _accum_target(param):
    """Where a parameter gradient may be ADDED in place by the producing kernel instead of being returned to autograd
    (which would allocate it and add it into .grad with one more pass): plain backward only (under create_graph the
    gradient must stay a differentiable tensor), leaf parameter with a pre-allocated contiguous fp32 .grad."""
    if param is None or torch.is_grad_enabled():
        return None
    if not (param.is_leaf and param.requires_grad):
        return None
    g = param.grad
    if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != param.shape:
        return None
    return g


_DERIVED_SLICES = not config.flag("GS_NO_DERIVED_SLICES")   # A/B switch for measurements


class _WeightSlice(Function):
    """w[:, :, lo:hi, :] as a contiguous kernel operand (the 257-input-channel conv of the last discriminator block is evaluated
    as two convs on slices of one variable).  Plain backward: the slice's gradient is added straight into that slice of w.grad
    (one launch) instead of autograd's zero-filled full-size tensor + copy + accumulate (three)."""

    @staticmethod
    def forward(ctx, w, lo, hi):
        ctx.lo, ctx.hi, ctx.wref = lo, hi, w
        ctx.set_materialize_grads(False)   # (the convs add their gradients into the slice of w.grad themselves and hand None back: without this
        K = _K()                           #  the engine calls backward with zeros -- a fill and a strided add of nothing per slice and pass)
        if _DERIVED_SLICES and hasattr(K, "derived_slice"):   # persistent copy, refreshed with the parameter (kernels.derived_slice)
            return K.derived_slice(w, lo, hi)
        return w[:, :, lo:hi, :].contiguous()

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        tgt = _accum_target(ctx.wref)
        if tgt is not None:
            # This node runs on the stream of ITS forward: with the real and the fake pass of a discriminator run on two streams, two of these
            # adds -- read-modify-writes of the same slice of w.grad -- met unordered: one contribution lost in ~2 % of the replayed fp32
            # iterations (scripts/dbg_race.py; round 6).  Ordered like every other launch that adds into a gradient at once.
            view = tgt[:, :, ctx.lo:ctx.hi, :]
            K = _K()
            with (K._adds_into(view) if hasattr(K, "_adds_into") else contextlib.nullcontext()):
                view.add_(g)
            return None, None, None
        return torch.nn.functional.pad(g, (0, 0, ctx.lo, ctx.wref.shape[2] - ctx.hi)), None, None


def weight_slice(w, lo, hi):
    t = _WeightSlice.apply(w, lo, hi)
    t._gs_slice_of = (w, lo, hi)   # lets the conv's backward add its gradient straight into that slice of w.grad (_slice_target)
    return t


def _slice_target(wref, x, gy, kind):
    """w.grad[:, :, lo:hi, :] (a strided view) when `wref` is a channel slice of a variable and the kernel layer can add a conv
    weight gradient into such a view (deferred, grouped layers: kernels.wgrad_slice_target_ok); None otherwise -- the gradient
    then goes back through _WeightSlice.backward."""
    src = getattr(wref, "_gs_slice_of", None)
    K = _K()
    if src is None or not isinstance(kind, _ConvKind) or not hasattr(K, "wgrad_slice_target_ok"):
        return None
    if not K.wgrad_slice_target_ok(x, gy.shape[1], kind.ksize, kind.stride):
        return None
    g = _accum_target(src[0])
    return None if g is None else g[:, :, src[1]:src[2], :]


# ---- "premasked" gradients ------------------------------------------------------------------------------------------------
# A block z = act(conv(..) + b) has the backward gy = gz * act'(z) followed by the conv gradients.  When z has ONE consumer (the
# caller says so: `in_act` of the consuming op -- networks.py knows its own wiring) and that consumer is a conv or a pixel norm,
# the multiplication by act'(z) moves into the kernel that produces gz (its input x IS z): one full read-modify-write pass per
# activation disappears from the plain backward.  The consumer tells the producer through the producer's ctx (= z.grad_fn)
# which tensor is already masked; under create_graph nothing is fused (the pieces must stay differentiable Functions).
_NO_PREMASK = config.flag("GS_NO_PREMASK")   # A/B switches for measurements
_NO_PREMASK_GRAPH = config.flag("GS_NO_PREMASK_GRAPH")
_NO_PREMASK_GRAPH2 = config.flag("GS_NO_PREMASK_GRAPH2")


def _premask_producer(x, in_act, differentiable=False):
    """ctx of the _ConvBiasAct that produced x when the fused path applies, else None.  Under create_graph only the
    `differentiable` caller (which then uses _BwdDataMasked) and only for leaky relu."""
    if in_act == ACT_NONE or _NO_PREMASK:
        return None
    if torch.is_grad_enabled() and not (differentiable and in_act == ACT_LRELU and not _NO_PREMASK_GRAPH):
        return None
    fn = x.grad_fn
    if fn is not None and getattr(fn, "_gs_act_out", ACT_NONE) == in_act:
        return fn
    return None


def _take_premasked(ctx, gz):
    """True when the incoming gradient is the tensor a consumer marked as already multiplied by act'(z)."""
    ptr = getattr(ctx, "_gs_premasked", None)
    ctx._gs_premasked = None
    return ptr is not None and ptr == gz.data_ptr()


_KINDS = {}


def _kind(key):
    if key not in _KINDS:
        if key[0] == "conv":
            _KINDS[key] = _ConvKind(key[1], key[2])
        elif key[0] == "convT":
            _KINDS[key] = _ConvTransposeKind()
        elif key[0] == "dense_flat":
            _KINDS[key] = _DenseFlatKind()
        else:
            _KINDS[key] = _DenseKind()
    return _KINDS[key]


class _Bilinear(Function):
    """y = alpha * B(x, w)."""

    @staticmethod
    def forward(ctx, x, w, kind, alpha):
        ctx.kind, ctx.alpha, ctx.wref = kind, alpha, w
        ctx.save_for_backward(x, w)
        return kind.fwd(x, w, alpha)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gx = _BilinearBwdData.apply(gy, w, x.shape, ctx.kind, ctx.alpha) if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[1] and _want_params():
            tgt = _accum_target(ctx.wref)
            if tgt is None:
                tgt = _slice_target(ctx.wref, x, gy, ctx.kind)
            if tgt is not None:
                ctx.kind.bwd_weight(x, gy, ctx.alpha, out=tgt)
            else:
                gw = _BilinearBwdWeight.apply(x, gy, ctx.kind, ctx.alpha).to(w.dtype)
        return gx, gw, None, None


class _BilinearBwdData(Function):
    """gx = alpha * d<gy, B(x,w)>/dx   (linear in gy and in w)."""

    @staticmethod
    def forward(ctx, gy, w, x_shape, kind, alpha, sole_consumer=False):
        ctx.kind, ctx.alpha, ctx.wref = kind, alpha, w
        ctx.sole_consumer = bool(sole_consumer)   # gy comes straight out of a _PnActBwd node and feeds nothing else (caller's promise)
        ctx.save_for_backward(gy, w)
        # (the end of the R1 pass's chain of _BwdDataMasked nodes -- the colour block's data gradient: see _BwdDataMasked.forward)
        up = gy.grad_fn
        ctx._gs_up = up if (isinstance(up, _BwdDataMasked._backward_cls) and not _want_params() and hasattr(kind, "fwd_mask") and not _NO_PREMASK_GRAPH2) else None
        return kind.bwd_data(gy, w, x_shape, alpha)

    @staticmethod
    def backward(ctx, ggx):
        gy, w = ctx.saved_tensors
        g_gy = None
        if ctx.needs_input_grad[0]:
            pn = gy.grad_fn if (_FUSE_NORM_BWD2 and ctx.sole_consumer and not torch.is_grad_enabled() and hasattr(ctx.kind, "fwd_pnbwdbwd")) else None
            if (pn is not None and isinstance(pn, _PnActBwd._backward_cls) and pn.needs_input_grad[0] and pn.needs_input_grad[1]
                    and ctx.kind.fwd_pnbwdbwd_is_fused(tuple(ggx.shape), gy.shape[1], gy.dtype)):
                # second-order pass: B(ggx, w) is the cotangent of that node's output, and both of its gradients come out of the conv's
                # epilogue; the node finds them under the address of what it is handed (see _PnActBwd.backward)
                g, z = pn.saved_tensors
                g_z, g_gy = ctx.kind.fwd_pnbwdbwd(ggx, w, ctx.alpha, g, z, pn.eps, pn.act)
                if _CHECK_FUSION:
                    _check_fused("fwd_pnbwdbwd", (g_z, g_gy), _K().pixel_norm_bwd_bwd(ctx.kind.fwd(ggx, w, ctx.alpha), g, z, pn.eps, pre_act=pn.act, with_g=True))
                pn._gs_done = (g_gy.data_ptr(), g_z)
            elif ctx._gs_up is not None and not torch.is_grad_enabled():
                up = ctx._gs_up   # the node that produced gy multiplies its cotangent by its mask first: in this conv's epilogue instead
                g_gy = ctx.kind.fwd_mask(ggx, w, ctx.alpha, up.saved_tensors[2], up.act)
                if _CHECK_FUSION:
                    _check_fused("fwd_mask", g_gy, _K().act_bwd(ctx.kind.fwd(ggx, w, ctx.alpha), up.saved_tensors[2], up.act))
                up._gs_gg_premasked = g_gy.data_ptr()
            else:
                g_gy = _Bilinear.apply(ggx, w, ctx.kind, ctx.alpha)
        g_w = None
        if ctx.needs_input_grad[1]:
            tgt = _accum_target(ctx.wref)
            if tgt is None:
                tgt = _slice_target(ctx.wref, ggx, gy, ctx.kind)
            if tgt is not None:   # second-order term of the penalty, added straight into w.grad
                ctx.kind.bwd_weight(ggx, gy, ctx.alpha, out=tgt)
            else:
                g_w = _BilinearBwdWeight.apply(ggx, gy, ctx.kind, ctx.alpha).to(w.dtype)
        return g_gy, g_w, None, None, None, None


class _BwdDataMasked(Function):
    """u = m * B^T(gy, w) with m = act'(.) through x, the (piecewise-linear) activation output that was the conv's input: the
    data gradient w.r.t. the previous layer's PRE-activation in one launch, under create_graph (the first-order pass of the R1
    penalty).  m is constant, so u is bilinear in (gy, w) like B^T itself: d<gg, u>/dgy = B(m gg, w), d<gg, u>/dw =
    bwd_weight(m gg, gy).  Leaky relu only (a smooth activation would add a term through m)."""

    @staticmethod
    def forward(ctx, gy, w, x, kind, alpha, act):
        if act != ACT_LRELU:
            raise NotImplementedError("_BwdDataMasked: piecewise-linear activations only")
        ctx.kind, ctx.alpha, ctx.act, ctx.wref = kind, alpha, act, w
        ctx.save_for_backward(gy, w, x)
        # The chain of these nodes runs in reverse in the second-order pass: this node's backward hands B(m gg, w) to the node that
        # produced gy, whose first step is to multiply by ITS mask (its x).  When gy comes straight from such a node and feeds
        # nothing else (data-gradients-only pass), that multiplication moves into this node's conv epilogue.
        up = gy.grad_fn
        ctx._gs_up = up if (isinstance(up, _BwdDataMasked._backward_cls) and not _want_params() and hasattr(kind, "fwd_mask") and not _NO_PREMASK_GRAPH2) else None
        ctx._gs_gg_premasked = None
        return kind.bwd_data_mask(gy, w, x.shape, alpha, x, act)

    @staticmethod
    def backward(ctx, gg):
        gy, w, x = ctx.saved_tensors
        pre, ctx._gs_gg_premasked = ctx._gs_gg_premasked, None
        if pre is not None and pre != gg.data_ptr():
            _handoff_broken("activation mask of the R1 chain in the producing conv")
        if pre is not None and not torch.is_grad_enabled():
            t = gg                                   # the producer of gg already applied this node's mask
        else:
            t = _ActBwd.apply(gg, x, ctx.act)
        up = ctx._gs_up
        if up is not None and ctx.needs_input_grad[0] and not torch.is_grad_enabled():
            g_gy = ctx.kind.fwd_mask(t, w, ctx.alpha, up.saved_tensors[2], up.act)
            if _CHECK_FUSION:
                _check_fused("fwd_mask", g_gy, _K().act_bwd(ctx.kind.fwd(t, w, ctx.alpha), up.saved_tensors[2], up.act))
            up._gs_gg_premasked = g_gy.data_ptr()
        else:
            g_gy = _Bilinear.apply(t, w, ctx.kind, ctx.alpha) if ctx.needs_input_grad[0] else None
        g_w = None
        if ctx.needs_input_grad[1]:
            tgt = _accum_target(ctx.wref)
            if tgt is None:
                tgt = _slice_target(ctx.wref, t, gy, ctx.kind)
            if tgt is not None:   # second-order term of the penalty, added straight into w.grad
                ctx.kind.bwd_weight(t, gy, ctx.alpha, out=tgt)
            else:
                g_w = _BilinearBwdWeight.apply(t, gy, ctx.kind, ctx.alpha).to(w.dtype)
        return g_gy, g_w, None, None, None, None


class _BilinearBwdWeight(Function):
    """gw = alpha * d<gy, B(x,w)>/dw   (linear in x and in gy); fp32 out."""

    @staticmethod
    def forward(ctx, x, gy, kind, alpha):
        ctx.kind, ctx.alpha = kind, alpha
        ctx.save_for_backward(x, gy)
        return kind.bwd_weight(x, gy, alpha)

    @staticmethod
    def backward(ctx, ggw):
        x, gy = ctx.saved_tensors
        g_x = _BilinearBwdData.apply(gy, ggw, x.shape, ctx.kind, ctx.alpha) if ctx.needs_input_grad[0] else None
        g_gy = _Bilinear.apply(x, ggw, ctx.kind, ctx.alpha) if ctx.needs_input_grad[1] else None
        return g_x, g_gy, None, None


def _bias_act_backward(gz, z, act, bias_param, want_b):
    """Backward of z = act(y + bias): (gy, gb).  Plain backward: one fused pass, the bias gradient added straight into
    bias.grad when possible (gb = None then).  Under create_graph: differentiable Functions."""
    plain = not torch.is_grad_enabled()
    tgt = _accum_target(bias_param) if want_b else None
    if act != ACT_NONE:
        if want_b and plain:
            gy, gb = _K().act_bwd_bias(gz, z, act, out=tgt)
            return gy, (None if tgt is not None else gb)
        gy = _ActBwd.apply(gz, z, act)
        return gy, (_ChannelSum.apply(gy) if want_b else None)
    if want_b and tgt is not None:
        _K().channel_sum(gz, out=tgt)
        return gz, None
    return gz, (_ChannelSum.apply(gz) if want_b else None)


class _ConvBiasAct(Function):
    """z = act(alpha * B(x, w) + bias) with the bias / activation fused into the GEMM epilogue."""

    @staticmethod
    def forward(ctx, x, w, bias, kind, alpha, act, in_act=ACT_NONE, input_normed=False):
        ctx.kind, ctx.alpha, ctx.act, ctx.has_bias = kind, alpha, act, bias is not None
        ctx.wref, ctx.bref = w, bias
        ctx.in_act = in_act        # x is the single-consumer output of that activation (caller's promise)
        ctx.input_normed = bool(input_normed)   # x is pixel_norm(.) out of a _ConvBiasActNorm node, this conv its only consumer (see _GZ)
        ctx._gs_act_out = act      # what consumers of z may fold into their own kernels
        ctx._gs_premasked = None
        z = kind.fwd_bias_act(x, w, bias, alpha, act)
        _tap(z, act)
        ctx.save_for_backward(x, w, z)
        return z

    @staticmethod
    def backward(ctx, gz):
        x, w, z = ctx.saved_tensors
        want_w = ctx.needs_input_grad[1] and _want_params()
        want_b = ctx.has_bias and ctx.needs_input_grad[2] and _want_params()
        act = ACT_NONE if _take_premasked(ctx, gz) else ctx.act   # (a consumer of z already applied act'(z))

        def data_grad(gy):
            if not ctx.needs_input_grad[0]:
                return None
            if _PARAMS_ONLY and x.grad_fn is None and not torch.is_grad_enabled():
                return None   # x is a leaf (the image batch of the R1 term) and this backward pass is after parameter gradients only
            if _FUSE_NORM_BWD and ctx.input_normed and not torch.is_grad_enabled() and hasattr(ctx.kind, "bwd_data_pnbwd"):
                pn = x.grad_fn   # the generator block whose normalised output this conv reads: its norm / activation backward in this conv's data gradient
                if (isinstance(pn, _ConvBiasActNorm._backward_cls) and pn.act in (ACT_NONE, ACT_LRELU)
                        and ctx.kind.bwd_data_pnbwd_is_fused(tuple(x.shape), gy.shape[1], gy.dtype)):
                    z_prev = pn.saved_tensors[2]
                    gz_prev = _GZ.pop(z_prev.data_ptr(), None)
                    gx_ = ctx.kind.bwd_data_pnbwd(gy, w, tuple(x.shape), ctx.alpha, z_prev, pn.eps, pn.act, gz_prev)
                    if _CHECK_FUSION:
                        _check_fused("bwd_data_pnbwd", gx_, _K().pixel_norm_bwd(ctx.kind.bwd_data(gy, w, tuple(x.shape), ctx.alpha), z_prev, pn.eps, act=pn.act, addend=gz_prev))
                    pn._gs_fused = (gx_.data_ptr(), gz_prev is not None)
                    return gx_
            prod = _premask_producer(x, ctx.in_act, differentiable=True) if hasattr(ctx.kind, "bwd_data_mask") else None
            if prod is None:
                return _BilinearBwdData.apply(gy, w, x.shape, ctx.kind, ctx.alpha)
            if torch.is_grad_enabled():   # create_graph: the same fusion as a differentiable Function
                gx_ = _BwdDataMasked.apply(gy, w, x, ctx.kind, ctx.alpha, ctx.in_act)
            else:
                gx_ = ctx.kind.bwd_data_mask(gy, w, x.shape, ctx.alpha, x, ctx.in_act)
            prod._gs_premasked = gx_.data_ptr()
            return gx_

        if want_b and want_w and getattr(ctx.kind, "bias_in_wgrad", False):
            tw, tb = _accum_target(ctx.wref), _accum_target(ctx.bref)
            if tw is not None and tb is not None:   # plain backward: weight and bias gradients from the same launches
                gy = _ActBwd.apply(gz, z, act) if act != ACT_NONE else gz
                gx = data_grad(gy)
                ctx.kind.bwd_weight(x, gy, ctx.alpha, out=tw, bias_out=tb)
                return gx, None, None, None, None, None, None, None
        gy, gb = _bias_act_backward(gz, z if act != ACT_NONE else None, act, ctx.bref if want_b else None, want_b)
        gx = data_grad(gy)
        gw = None
        if want_w:
            tgt = _accum_target(ctx.wref)
            if tgt is not None:
                ctx.kind.bwd_weight(x, gy, ctx.alpha, out=tgt)
            else:
                gw = _BilinearBwdWeight.apply(x, gy, ctx.kind, ctx.alpha).to(w.dtype)
        return gx, gw, gb, None, None, None, None, None


class _PnActBwd(Function):
    """u = act'(z) * pixel_norm_bwd(g, z): the backward of (activation -> pixel norm) w.r.t. the pre-activation in ONE kernel,
    differentiable once more (mode-seeking term): with M = diag(act'(z)) constant (leaky relu) and J(z) the symmetric Jacobian
    of the norm, u = M J g, so  du/dg^T gg = J (M gg)  and  du/dz^T gg = d<M gg, J g>/dz  -- the norm's own first- and
    second-order kernels with the mask folded in on the input side."""

    @staticmethod
    def forward(ctx, g, z, eps, act):
        if act != ACT_LRELU:
            raise NotImplementedError("_PnActBwd: piecewise-linear activations only (the tanh head has no pixel norm)")
        ctx.eps, ctx.act = eps, act
        ctx._gs_done = None
        ctx.save_for_backward(g, z)
        return _K().pixel_norm_bwd(g, z, eps, act=act)

    @staticmethod
    @once_differentiable
    def backward(ctx, gg):
        g, z = ctx.saved_tensors
        done, ctx._gs_done = ctx._gs_done, None
        if ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:   # both from one pass over gg, g, z
            if done is not None and gg.data_ptr() != done[0]:
                _handoff_broken("second-order norm gradients in the forward-on-cotangent conv")
            if done is not None:
                g_g, g_z = gg, done[1]   # the conv that produced this node's cotangent already went through it (_BilinearBwdData.backward)
            else:
                g_z, g_g = _K().pixel_norm_bwd_bwd(gg, g, z, ctx.eps, pre_act=ctx.act, with_g=True)
            if _FUSE_NORM_BWD:
                _GZ[z.data_ptr()] = g_z   # (see above: the consumer of pixel_norm(z) may add it in its data-gradient epilogue)
            return g_g, g_z, None, None
        if done is not None:
            _handoff_broken("second-order norm gradients in the forward-on-cotangent conv")
        g_g = _K().pixel_norm_bwd(gg, z, ctx.eps, pre_act=ctx.act) if ctx.needs_input_grad[0] else None
        g_z = _K().pixel_norm_bwd_bwd(gg, g, z, ctx.eps, pre_act=ctx.act) if ctx.needs_input_grad[1] else None
        return g_g, g_z, None, None


_FUSE_NORM_EPILOGUE = not config.flag("GS_NO_NORM_EPILOGUE")   # A/B switch for measurements
_FUSE_NORM_BWD = not config.flag("GS_NO_NORM_BWD_EPILOGUE")  # A/B switch: the previous block's norm backward in the data-gradient epilogue
_FUSE_NORM_BWD2 = not config.flag("GS_NO_NORM_BWD2_EPILOGUE")  # A/B switch: the norm's second-order kernel in the forward-on-cotangent conv

# ---- the previous block's (activation -> pixel norm) backward inside the conv that produces its input gradient -----------------------
# Plain backward of a generator block: g_y -> [pixel_norm_bwd(g_y, z) + g_z] * act'(z) -> data gradient conv -> g_y of the block before.
# Where the conv's tile owns every channel of a pixel (the 32- / 64-channel layers) that elementwise pass (4 tensors) runs in the
# epilogue of the conv of the block AFTER (gs_conv2d[_transpose_s2]_bwd_data_pnbwd).  The consumer does it when the caller promised
# that its input feeds nothing else (`input_normed`, networks.py), the producer is a _ConvBiasActNorm node and the shape has the epilogue
# form; it tells the producer through its ctx (`_gs_fused`) which incoming tensor is already the gradient w.r.t. its pre-activation.
# g_z -- the gradient the second-order graph of the mode-seeking term sends into z -- belongs to the PRODUCER's inputs; its kernel
# (_PnActBwd.backward) leaves it here as well, keyed by z's address, and it is always there in time: that kernel of block L runs before
# the one of block L + 1, whose result the consumer's own backward waits for.  Cleared per backward pass (reset_fusion_state).
_GZ = {}


def reset_fusion_state():
    _GZ.clear()


# The cross-node hand-offs above (and `_gs_done`, `_gs_gg_premasked`) rest on caller promises ("this tensor has ONE consumer").  A broken
# promise shows as a marked node receiving a DIFFERENT tensor than the one its partner produced (autograd summed a second gradient into
# it): that is an error, never a silent fallback -- the partner's tensor already went through this node's arithmetic.
def _handoff_broken(what):
    raise RuntimeError("gansynth_amd.functional: fused hand-off '%s' was prepared but the node received another tensor -- the single-consumer "
                       "promise of the wiring (networks.py: input_normed / input_activation, functional: sole_consumer) does not hold" % what)


# GS_CHECK_FUSION=1: every fused cross-node form also runs its unfused definition and the two are compared (debug mode).
_CHECK_FUSION = config.flag("GS_CHECK_FUSION")


def _check_fused(what, got, ref):
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return   # (the comparison reads values back: eager passes only -- every captured pass has an eager warm-up twin)
    for g, r in zip(got if isinstance(got, (tuple, list)) else (got,), ref if isinstance(ref, (tuple, list)) else (ref,)):
        scale = float(r.float().abs().max()) + 1e-30
        err = float((g.float() - r.float()).abs().max()) / scale
        tol = 1e-4 if g.dtype == torch.float32 else 4e-2
        if not err <= tol:
            raise RuntimeError("GS_CHECK_FUSION: %s differs from its unfused definition by %.3e of the tensor's scale" % (what, err))

_NORM_BWD_BIAS = not config.flag("GS_NO_NORM_BWD_BIAS")      # A/B switch: bias sums inside the norm's backward


class _ConvBiasActNorm(Function):
    """(y, z) with z = act(alpha * B(x, w) + bias), y = pixel_norm(z): a generator block as one node.  z is returned only so
    that second-order graphs built on it (the norm's backward is differentiated by the mode-seeking term) send their gradient
    back here: the plain backward then forms (pixel_norm_bwd(g_y, z) + g_z) * act'(z) in one pass instead of
    norm-backward, add, activation-backward."""

    @staticmethod
    def forward(ctx, x, w, bias, kind, alpha, act, eps, input_normed=False):
        ctx.kind, ctx.alpha, ctx.act, ctx.eps, ctx.has_bias = kind, alpha, act, eps, bias is not None
        ctx.wref, ctx.bref = w, bias
        ctx.input_normed = bool(input_normed)   # x is pixel_norm(.) out of a _ConvBiasActNorm node and feeds nothing but this conv (caller's promise)
        ctx._gs_fused = None
        ctx.set_materialize_grads(False)   # an absent gradient for z must arrive as None, not as a tensor of zeros
        keep = any(ctx.needs_input_grad)   # no backward (the no-grad generator pass of the D run): the activation is not kept
        want_z = keep or activation_tap.active is not None
        if _FUSE_NORM_EPILOGUE:
            z, y = kind.fwd_bias_act_norm(x, w, bias, alpha, act, eps, want_z)
        else:
            z = kind.fwd_bias_act(x, w, bias, alpha, act)
            y = _K().pixel_norm_fwd(z, eps)
        if want_z:
            _tap(z, act)
        if keep:
            ctx.save_for_backward(x, w, z)
        return y, z

    @staticmethod
    def backward(ctx, g_y, g_z):
        x, w, z = ctx.saved_tensors
        want_w = ctx.needs_input_grad[1] and _want_params()
        want_b = ctx.has_bias and ctx.needs_input_grad[2] and _want_params()
        if torch.is_grad_enabled():   # create_graph: differentiable pieces
            gy = _PnActBwd.apply(g_y, z, ctx.eps, ctx.act) if g_y is not None else None
            if g_z is not None:
                extra = _ActBwd.apply(g_z, z, ctx.act)
                gy = extra if gy is None else gy + extra
            sole = g_y is not None and g_z is None and not want_w and not want_b   # gy: straight out of _PnActBwd, into the data gradient only
            gx = _BilinearBwdData.apply(gy, w, x.shape, ctx.kind, ctx.alpha, sole) if ctx.needs_input_grad[0] else None
            gw = _BilinearBwdWeight.apply(x, gy, ctx.kind, ctx.alpha).to(w.dtype) if want_w else None
            gb = _ChannelSum.apply(gy) if want_b else None
            return gx, gw, gb, None, None, None, None, None
        tw = _accum_target(ctx.wref) if want_w else None
        tb = _accum_target(ctx.bref) if want_b else None
        bias_done = False
        fused, ctx._gs_fused = ctx._gs_fused, None
        if fused is not None and (g_y is None or g_y.data_ptr() != fused[0]):
            _handoff_broken("previous block's norm backward in the data-gradient conv")
        if fused is not None:
            # the consumer's data-gradient conv already went through this block's norm and activation (and added g_z if it had it)
            gy = g_y
            if g_z is not None and not fused[1]:
                gy = _K().axpby(gy, _K().act_bwd(g_z, z, ctx.act), 1.0, 1.0)
        elif g_y is None:
            gy = _K().act_bwd(g_z, z, ctx.act)
        elif (tb is not None and not getattr(ctx.kind, "bias_in_wgrad", False) and _NORM_BWD_BIAS and getattr(_K(), "norm_bwd_sums_bias", False)
              and _K().norm_bwd_bias_ok(z.shape[1], z.dtype)):   # (other channel counts, e.g. 48 or 96: plain backward + channel_sum below)
            # (blocks whose weight-gradient kernel carries no bias row -- the transposed convs: the norm's backward sums its own result)
            gy = _K().pixel_norm_bwd(g_y, z, ctx.eps, act=ctx.act, addend=g_z, bias_out=tb)
            bias_done = True
        else:
            gy = _K().pixel_norm_bwd(g_y, z, ctx.eps, act=ctx.act, addend=g_z)
        gx = None
        if ctx.needs_input_grad[0]:
            prod = x.grad_fn if (_FUSE_NORM_BWD and ctx.input_normed and hasattr(ctx.kind, "bwd_data_pnbwd")) else None
            if (prod is not None and isinstance(prod, _ConvBiasActNorm._backward_cls) and prod.act in (ACT_NONE, ACT_LRELU)
                    and ctx.kind.bwd_data_pnbwd_is_fused(tuple(x.shape), gy.shape[1], gy.dtype)):
                z_prev = prod.saved_tensors[2]
                gz_prev = _GZ.pop(z_prev.data_ptr(), None)
                gx = ctx.kind.bwd_data_pnbwd(gy, w, tuple(x.shape), ctx.alpha, z_prev, prod.eps, prod.act, gz_prev)
                if _CHECK_FUSION:
                    _check_fused("bwd_data_pnbwd", gx, _K().pixel_norm_bwd(ctx.kind.bwd_data(gy, w, tuple(x.shape), ctx.alpha), z_prev, prod.eps, act=prod.act, addend=gz_prev))
                prod._gs_fused = (gx.data_ptr(), gz_prev is not None)
            else:
                gx = _BilinearBwdData.apply(gy, w, x.shape, ctx.kind, ctx.alpha)
        gw = gb = None
        if bias_done:
            want_b = False
        if tw is not None and tb is not None and getattr(ctx.kind, "bias_in_wgrad", False):
            ctx.kind.bwd_weight(x, gy, ctx.alpha, out=tw, bias_out=tb)
            return gx, None, None, None, None, None, None, None
        if want_b:
            if tb is not None:
                _K().channel_sum(gy, out=tb)
            else:
                gb = _K().channel_sum(gy)
        if want_w:
            if tw is not None:
                ctx.kind.bwd_weight(x, gy, ctx.alpha, out=tw)
            else:
                gw = ctx.kind.bwd_weight(x, gy, ctx.alpha).to(w.dtype)
        return gx, gw, gb, None, None, None, None, None


def conv2d_bias_act_norm(x, w, bias, ksize, stride, alpha, act, eps, input_normed=False):
    return _ConvBiasActNorm.apply(x, w, bias, _kind(("conv", ksize, stride)), alpha, act, eps, input_normed)[0]


def conv2d_transpose_bias_act_norm(x, w, bias, alpha, act, eps, input_normed=False):
    return _ConvBiasActNorm.apply(x, w, bias, _kind(("convT",)), alpha, act, eps, input_normed)[0]


def conv2d(x, w, ksize, stride, alpha):
    return _Bilinear.apply(x, w, _kind(("conv", ksize, stride)), alpha)


def conv2d_bias_act(x, w, bias, ksize, stride, alpha, act, in_act=ACT_NONE, input_normed=False):
    return _ConvBiasAct.apply(x, w, bias, _kind(("conv", ksize, stride)), alpha, act, in_act, input_normed)


def conv2d_transpose_bias_act(x, w, bias, alpha, act):
    return _ConvBiasAct.apply(x, w, bias, _kind(("convT",)), alpha, act, ACT_NONE)


def conv2d_transpose(x, w, alpha):
    return _Bilinear.apply(x, w, _kind(("convT",)), alpha)


def dense(x, w, alpha):
    return _Bilinear.apply(x, w, _kind(("dense",)), alpha)


def dense_bias_act(x, w, bias, alpha, act):
    """act(alpha * x @ w + bias) (ops.py:183-201 as one node: the bias / activation ride where the forward writes its result).  x: [b, in], or
    a channels-last 4-D activation whose NCHW flatten feeds the layer (networks.py:185-186) where the kernel layer takes it as it is."""
    K = _K()
    if x.dim() == 4:
        if hasattr(K, "dense_nhwc_ok") and K.dense_nhwc_ok(x, w.shape[1]):
            return _ConvBiasAct.apply(x, w, bias, _kind(("dense_flat",)), alpha, act)
        x = x.reshape(x.shape[0], -1)
    return _ConvBiasAct.apply(x, w, bias, _kind(("dense",)), alpha, act)


def dense_of_flattened(x, w, alpha):
    """dense(tf.layers.flatten(x), w) for a 4-D activation: without the NCHW copy where the kernel layer can read the channels-last
    memory directly, the plain reshape + dense otherwise."""
    K = _K()
    if hasattr(K, "dense_nhwc_ok") and x.dim() == 4 and K.dense_nhwc_ok(x, w.shape[1]):
        return _Bilinear.apply(x, w, _kind(("dense_flat",)), alpha)
    return dense(x.reshape(x.shape[0], -1), w, alpha)


# --------------------------------------------------------------------------- embedding
class _Embedding(Function):
    @staticmethod
    def forward(ctx, idx, w, alpha, dtype):
        ctx.alpha, ctx.rows = alpha, w.shape[0]
        ctx.save_for_backward(idx)
        return _K().embedding_fwd(idx, w, alpha, dtype)

    @staticmethod
    def backward(ctx, gy):
        (idx,) = ctx.saved_tensors
        return None, (_EmbeddingBwd.apply(idx, gy, ctx.rows, ctx.alpha) if _want_params() else None), None, None


class _EmbeddingBwd(Function):
    @staticmethod
    def forward(ctx, idx, gy, rows, alpha):
        ctx.alpha, ctx.dtype = alpha, gy.dtype
        ctx.save_for_backward(idx)
        return _K().embedding_bwd(idx, gy, rows, alpha)

    @staticmethod
    def backward(ctx, ggw):
        (idx,) = ctx.saved_tensors
        return None, _Embedding.apply(idx, ggw, ctx.alpha, ctx.dtype), None, None


def embedding(idx, w, alpha, dtype):
    return _Embedding.apply(idx, w, alpha, dtype)


class _EmbeddingOneHot(Function):
    """embedding(argmax(labels)) in one launch (the kernel finds the index itself and hands it to the backward)."""

    @staticmethod
    def forward(ctx, labels, w, alpha):
        ctx.alpha, ctx.rows = alpha, w.shape[0]
        y, idx = _K().embedding_onehot_fwd(labels, w, alpha)
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    def backward(ctx, gy):
        (idx,) = ctx.saved_tensors
        return None, (_EmbeddingBwd.apply(idx, gy, ctx.rows, ctx.alpha) if _want_params() else None), None


def embedding_onehot(labels, w, alpha):
    """ops.py:204-218 on one-hot rows; falls back to argmax + embedding where the kernel layer has no fused form."""
    if hasattr(_K(), "embedding_onehot_fwd") and labels.dtype in (torch.float32, torch.bfloat16):
        return _EmbeddingOneHot.apply(labels, w, alpha)
    return embedding(torch.argmax(labels, dim=1), w, alpha, labels.dtype)


# ------------------------------------------------------------------- bias + activation
class _ChannelSum(Function):
    @staticmethod
    def forward(ctx, g):
        ctx.shape, ctx.dtype = g.shape, g.dtype
        return _K().channel_sum(g)

    @staticmethod
    def backward(ctx, gs):
        view = (1, -1, 1, 1) if len(ctx.shape) == 4 else (1, -1)
        return gs.to(ctx.dtype).view(view).expand(ctx.shape)


class _BiasAct(Function):
    """z = act(x + bias[c])."""

    @staticmethod
    def forward(ctx, x, bias, act):
        z = _K().bias_act_fwd(x, bias, act)
        _tap(z, act)
        ctx.act = act
        ctx.has_bias = bias is not None
        ctx.bref = bias
        if act != ACT_NONE:
            ctx.save_for_backward(z)
        return z

    @staticmethod
    def backward(ctx, gz):
        want_b = ctx.has_bias and ctx.needs_input_grad[1] and _want_params()
        z = ctx.saved_tensors[0] if ctx.act != ACT_NONE else None
        gx, gb = _bias_act_backward(gz, z, ctx.act, ctx.bref if want_b else None, want_b)
        return (gx if ctx.needs_input_grad[0] else None), gb, None


class _ActBwd(Function):
    """gx = g * act'(.) written through the activation output z."""

    @staticmethod
    def forward(ctx, g, z, act):
        ctx.act = act
        ctx.save_for_backward(g, z)
        return _K().act_bwd(g, z, act)

    @staticmethod
    def backward(ctx, ggx):
        g, z = ctx.saved_tensors
        g_g = _ActBwd.apply(ggx, z, ctx.act) if ctx.needs_input_grad[0] else None
        g_z = None
        if ctx.act == ACT_TANH and ctx.needs_input_grad[1]:
            g_z = _K().tanh_bwd_bwd(ggx, g, z)  # leaky_relu is piecewise linear: no term
        return g_g, g_z, None


class _UnitsBiasActNHWC(Function):
    """z = act(y + bias) with y the dense layer's units [n, c h w] (channel-major, networks.py:51-54) and z the channels-last activation
    [n, c, h, w]: bias, activation and the change of order in one pass; the backward hands the dense kernels a gradient in the units' order."""

    @staticmethod
    def forward(ctx, y, bias, c, h, w, act):
        z = _K().units_bias_act_to_nhwc(y, bias, c, h, w, act)
        _tap(z, act)
        ctx.act, ctx.has_bias, ctx.bref = act, bias is not None, bias
        ctx.save_for_backward(z)
        return z

    @staticmethod
    def backward(ctx, gz):
        (z,) = ctx.saved_tensors
        want_b = ctx.has_bias and ctx.needs_input_grad[1] and _want_params()
        gu = _NHWCActBwdToUnits.apply(gz, z, ctx.act) if torch.is_grad_enabled() else _K().nhwc_act_bwd_to_units(gz, z, ctx.act)
        _, gb = _bias_act_backward(gu, None, ACT_NONE, ctx.bref if want_b else None, want_b)
        return (gu if ctx.needs_input_grad[0] else None), gb, None, None, None, None


class _NHWCActBwdToUnits(Function):
    """gu[n][u] = g[n][p][ch] act'(z[n][p][ch]); linear in g, and for the piecewise-linear activation constant in z."""

    @staticmethod
    def forward(ctx, g, z, act):
        if act == ACT_TANH:
            raise NotImplementedError("_NHWCActBwdToUnits: piecewise-linear activations only under create_graph")
        ctx.act = act
        ctx.save_for_backward(z)
        return _K().nhwc_act_bwd_to_units(g, z, act)

    @staticmethod
    @once_differentiable
    def backward(ctx, ggu):
        (z,) = ctx.saved_tensors
        n, c, h, w = z.shape
        return (_K().units_bias_act_to_nhwc(ggu, None, c, h, w, ctx.act, mask=z) if ctx.needs_input_grad[0] else None), None, None


def units_nhwc_ok():
    return hasattr(_K(), "units_bias_act_to_nhwc") and not config.flag("GS_NO_UNITS_NHWC")


def units_bias_act_nhwc(y, bias, c, h, w, act):
    return _UnitsBiasActNHWC.apply(y, bias, int(c), int(h), int(w), act)


def bias_act(x, bias, act):
    return _BiasAct.apply(x, bias, act)


# ------------------------------------------------------------------------- pixel norm
class _PixelNorm(Function):
    @staticmethod
    def forward(ctx, x, eps, in_act=ACT_NONE):
        ctx.eps, ctx.in_act = eps, in_act
        ctx.save_for_backward(x)
        return _K().pixel_norm_fwd(x, eps)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        prod = _premask_producer(x, ctx.in_act)
        if prod is not None:   # x = act(..) with this norm as its only consumer: gradient w.r.t. the pre-activation directly
            gx = _K().pixel_norm_bwd(g, x, ctx.eps, act=ctx.in_act)
            prod._gs_premasked = gx.data_ptr()
            return gx, None, None
        return _PixelNormBwd.apply(g, x, ctx.eps), None, None


class _PixelNormBwd(Function):
    @staticmethod
    def forward(ctx, g, x, eps):
        ctx.eps = eps
        ctx.save_for_backward(g, x)
        return _K().pixel_norm_bwd(g, x, eps)

    @staticmethod
    def backward(ctx, gg):
        g, x = ctx.saved_tensors
        g_g = _PixelNormBwd.apply(gg, x, ctx.eps) if ctx.needs_input_grad[0] else None  # symmetric Jacobian
        g_x = _K().pixel_norm_bwd_bwd(gg, g, x, ctx.eps) if ctx.needs_input_grad[1] else None
        return g_g, g_x, None


def pixel_norm(x, eps, in_act=ACT_NONE):
    return _PixelNorm.apply(x, eps, in_act)


# ------------------------------------------------------------------ upscale / block sum
class _Upscale(Function):
    @staticmethod
    def forward(ctx, x, fy, fx, scale):
        ctx.f = (fy, fx, scale)
        return _K().upscale2d(x, fy, fx, scale)

    @staticmethod
    def backward(ctx, g):
        return _BlockSum.apply(g, *ctx.f), None, None, None


class _BlockSum(Function):
    @staticmethod
    def forward(ctx, x, fy, fx, scale):
        ctx.f = (fy, fx, scale)
        return _K().blocksum2d(x, fy, fx, scale)

    @staticmethod
    def backward(ctx, g):
        return _Upscale.apply(g, *ctx.f), None, None, None


def upscale(x, fy, fx):
    return _Upscale.apply(x, fy, fx, 1.0)


def avg_pool(x, fy, fx):
    return _BlockSum.apply(x, fy, fx, 1.0 / float(fy * fx))


# ------------------------------------------------------------------------ batch stddev
def _sub_kw(sub):
    return {} if sub == 1 else {"sub": sub}   # (kernel layers without sub-batches keep their signatures)


class _BatchStddev(Function):
    @staticmethod
    def forward(ctx, x, eps, sub=1):
        ctx.eps, ctx.sub = eps, sub
        ctx.save_for_backward(x)
        return _K().batch_stddev_fwd(x, eps, **_sub_kw(sub))

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return _BatchStddevBwd.apply(gy, x, ctx.eps, None, ctx.sub), None, None


class _BatchStddevBwd(Function):
    """batch_stddev_bwd(gy, x) + addend (the other gradient into x, when the statistic was taken with a tap)."""

    @staticmethod
    def forward(ctx, gy, x, eps, addend=None, sub=1):
        ctx.eps, ctx.sub = eps, sub
        ctx.save_for_backward(gy, x)
        return _K().batch_stddev_bwd(gy, x, eps, addend=addend, **_sub_kw(sub))

    @staticmethod
    @once_differentiable
    def backward(ctx, ggx):
        gy, x = ctx.saved_tensors
        ggy, gx2 = _K().batch_stddev_bwd_bwd(ggx, gy, x, ctx.eps, **_sub_kw(ctx.sub))
        return ggy, gx2, None, (ggx if ctx.needs_input_grad[3] else None), None


def batch_stddev(x, eps):
    return _BatchStddev.apply(x, eps)


class _BatchStddevTap(Function):
    """(x, batch_stddev(x)) with x passed through: the caller hands the FIRST output to whatever else consumes x (the conv beside the
    statistic, networks.py:174-176), so that x has one consumer in the graph and the two gradients into it are summed inside the
    statistic's backward kernel instead of by the autograd engine (one launch per backward pass through the block).
    `sub`: x is that many batches concatenated (the statistic within each)."""

    @staticmethod
    def forward(ctx, x, eps, sub=1):
        ctx.eps, ctx.sub = eps, sub
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x)
        return x.view_as(x), _K().batch_stddev_fwd(x, eps, **_sub_kw(sub))

    @staticmethod
    def backward(ctx, gx, gs):
        (x,) = ctx.saved_tensors
        if gs is None:
            return gx, None, None
        return _BatchStddevBwd.apply(gs, x, ctx.eps, gx, ctx.sub), None, None   # (gx None: the statistic's gradient alone)


def batch_stddev_tap(x, eps, sub_batches=1):
    return _BatchStddevTap.apply(x, eps, int(sub_batches))


# --------------------------------------------------------------------------------- lerp
class DeviceLerp(object):
    """The fade-in weight t of `lerp(a, b, t) = t a + (1 - t) b` (networks.py:10-11) kept in device memory: it changes every step
    of the progressive schedule, and a by-value kernel scalar would be frozen into a captured hipGraph.  `weights()` gives the two
    coefficients as objects the kernel layer resolves to (table, index); float() of them is the current host value (what the CPU
    emulation of the tests uses).  Table = [t, 1 - t, 0, 1]."""

    class Coef(object):
        def __init__(self, owner, index):
            self.owner, self.index = owner, index

        def __float__(self):
            return float(self.owner.host[self.index])

    _SLOTS = 4

    def __init__(self, device):
        self.host = torch.tensor([0.0, 1.0, 0.0, 1.0], dtype=torch.float32)   # current value (float() of the coefficients reads it)
        self._cuda = torch.device(device).type == "cuda"
        # the async H2D copy reads its pinned source when the DMA executes, and with graph replay the host runs steps ahead of
        # the device: every set() stages through its own pinned slot, reused only after the copy that read it has completed
        self._ring = [self.host.clone().pin_memory() for _ in range(self._SLOTS)] if self._cuda else None
        self._done = [None] * self._SLOTS
        self._next = 0
        self.table = self.host.to(device)

    def set(self, t):
        self.host[0], self.host[1] = float(t), 1.0 - float(t)
        if not self._cuda:
            self.table.copy_(self.host)
            return
        i = self._next
        self._next = (i + 1) % self._SLOTS
        if self._done[i] is not None:
            self._done[i].synchronize()
        self._ring[i].copy_(self.host)
        self.table.copy_(self._ring[i], non_blocking=True)   # stream-ordered before the next launch / graph replay
        ev = torch.cuda.Event()
        ev.record()
        self._done[i] = ev

    def weights(self):
        return DeviceLerp.Coef(self, 0), DeviceLerp.Coef(self, 1)

    def zero(self):
        return DeviceLerp.Coef(self, 2)


class DeviceScalars(object):
    """A few fp32 scalars a captured hipGraph reads from device memory (the optimizers' bias-corrected step sizes: by-value kernel
    scalars would be frozen into the graph).  `set(values)` is stream-ordered ahead of the next launch / replay; same pinned ring as
    DeviceLerp (the host runs replays ahead of the device)."""

    _SLOTS = 4

    def __init__(self, device, n):
        self.host = torch.zeros(n, dtype=torch.float32)
        self._cuda = torch.device(device).type == "cuda"
        self._ring = [self.host.clone().pin_memory() for _ in range(self._SLOTS)] if self._cuda else None
        self._done = [None] * self._SLOTS
        self._next = 0
        self.table = self.host.to(device)

    def set(self, values):
        for i, v in enumerate(values):
            self.host[i] = float(v)   # (round-to-nearest fp32: what ctypes.c_float does to a by-value scalar)
        if not self._cuda:
            self.table.copy_(self.host)
            return
        i = self._next
        self._next = (i + 1) % self._SLOTS
        if self._done[i] is not None:
            self._done[i].synchronize()
        self._ring[i].copy_(self.host)
        self.table.copy_(self._ring[i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._done[i] = ev

    def ptr(self, index):
        return self.table.data_ptr() + 4 * int(index)


def _coef_zero(c):
    """0 in the same representation as coefficient c (a device-table entry stays a device-table entry)."""
    return c.owner.zero() if isinstance(c, DeviceLerp.Coef) else 0.0


class _Axpby(Function):
    @staticmethod
    def forward(ctx, a, b, ca, cb):
        ctx.c = (ca, cb)
        return _K().axpby(a, b, ca, cb)

    @staticmethod
    def backward(ctx, g):
        ca, cb = ctx.c

        def scaled(coef, first):   # (a plain 1.0: the gradient itself, no launch)
            if isinstance(coef, float) and coef == 1.0:
                return g
            return _Axpby.apply(g, g, coef, _coef_zero(coef)) if first else _Axpby.apply(g, g, _coef_zero(coef), coef)

        return (scaled(ca, True) if ctx.needs_input_grad[0] else None, scaled(cb, False) if ctx.needs_input_grad[1] else None, None, None)


def axpby(a, b, ca, cb):
    return _Axpby.apply(a, b, ca, cb)


# ------------------------------------------------------------------------------ GAN losses
_UNIT = {}


def unit_seed(device):
    """The constant 1.0 (fp32 scalar, one per device) the trainer seeds its losses with (torch.autograd.backward(loss, unit_seed)):
    a loss head that is handed THIS tensor returns its stored gradients as they are instead of scaling them by a device scalar
    (three to five launches per loss).  Created outside stream capture (models.GANSynth does, when it is built)."""
    key = str(torch.device(device))
    t = _UNIT.get(key)
    if t is None:
        t = _UNIT[key] = torch.ones((), dtype=torch.float32, device=device)
    return t


def _is_unit(g):
    t = _UNIT.get(str(g.device))
    return t is not None and g.dim() == 0 and g.dtype == torch.float32 and g.data_ptr() == t.data_ptr()


class _GanDLoss(Function):
    """L_D = mean(softplus(-r) + softplus(f) + penalty) with r / f the label logits (models.py:39-49, 65): loss and gradients in
    one launch; the backward scales the stored gradients by the incoming scalar.  First order only (the second-order terms of the
    step live in `penalty`'s own graph)."""

    @staticmethod
    def forward(ctx, real_logits, fake_logits, labels, penalty, penalty_weight):
        loss, g_real, g_fake, g_pen = _K().gan_d_loss(real_logits, fake_logits, labels, penalty, penalty_weight)
        ctx.has_penalty = penalty is not None
        ctx.save_for_backward(g_real, g_fake, g_pen if ctx.has_penalty else g_real)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g_real, g_fake, g_pen = ctx.saved_tensors
        want_pen = ctx.has_penalty and ctx.needs_input_grad[3]
        if _is_unit(g):   # the trainer's seed: d loss / d loss = 1
            return (g_real if ctx.needs_input_grad[0] else None, g_fake if ctx.needs_input_grad[1] else None, None, g_pen if want_pen else None, None)
        return (g_real * g.to(g_real.dtype) if ctx.needs_input_grad[0] else None,
                g_fake * g.to(g_fake.dtype) if ctx.needs_input_grad[1] else None, None, g_pen * g if want_pen else None, None)


class _GanGLoss(Function):
    """L_G = mean(softplus(-f) + weight / (sumsq + eps)) (models.py:57-64), same scheme."""

    @staticmethod
    def forward(ctx, fake_logits, labels, sumsq, weight, eps):
        loss, g_fake, g_sumsq = _K().gan_g_loss(fake_logits, labels, sumsq, weight, eps)
        ctx.has_ms = sumsq is not None
        ctx.save_for_backward(g_fake, g_sumsq if ctx.has_ms else g_fake)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g_fake, g_sumsq = ctx.saved_tensors
        want_ms = ctx.has_ms and ctx.needs_input_grad[2]
        if _is_unit(g):
            return (g_fake if ctx.needs_input_grad[0] else None, None, g_sumsq if want_ms else None, None, None)
        return (g_fake * g.to(g_fake.dtype) if ctx.needs_input_grad[0] else None, None, g_sumsq * g if want_ms else None, None, None)


class _GanGLossModeSeeking(Function):
    """The mode-seeking half of L_G: mean(weight / (sumsq + eps)) (models.py:57-64): needs nothing of the discriminator."""

    @staticmethod
    def forward(ctx, sumsq, weight, eps):
        loss, _, g_sumsq = _K().gan_g_loss(None, None, sumsq, weight, eps)
        ctx.save_for_backward(g_sumsq)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (g_sumsq,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return (g_sumsq if _is_unit(g) else g_sumsq * g), None, None


def gan_g_loss_mode_seeking(sumsq, weight, eps):
    return _GanGLossModeSeeking.apply(sumsq, float(weight), float(eps))


class _GanDLossPair(Function):
    """_GanDLoss on ONE logits tensor holding the real batch's rows followed by the fake batch's (the discriminator tail run once over
    both, models.GANSynth._d_losses_b): same kernel, the two gradients written into the halves of one tensor."""

    @staticmethod
    def forward(ctx, logits, labels, penalty, penalty_weight):
        n = logits.shape[0] // 2
        g = torch.empty_like(logits)
        loss, _, _, g_pen = _K().gan_d_loss(logits[:n], logits[n:], labels, penalty, penalty_weight, out=(g[:n], g[n:]))
        ctx.has_penalty = penalty is not None
        ctx.save_for_backward(g, g_pen if ctx.has_penalty else g)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g_logits, g_pen = ctx.saved_tensors
        want_pen = ctx.has_penalty and ctx.needs_input_grad[2]
        if _is_unit(g):
            return g_logits if ctx.needs_input_grad[0] else None, None, g_pen if want_pen else None, None
        return g_logits * g.to(g_logits.dtype) if ctx.needs_input_grad[0] else None, None, g_pen * g if want_pen else None, None


def gan_d_loss_pair(logits, labels, penalty, penalty_weight=1.0):
    return _GanDLossPair.apply(logits, labels, penalty, float(penalty_weight))


def _cat2(a, b):
    """[a; b] along the batch axis, either half absent = zeros."""
    ref = a if a is not None else b
    n = ref.shape[0]
    cl = ref.dim() == 4
    if ref.is_cuda and (a is None or b is None or (a.stride() == b.stride() and a.dtype == b.dtype)):
        # ONE launch (torch.cat keeps the common memory format of its inputs): an absent half is a constant tensor of zeros, made once
        if a is None or b is None:
            key = (tuple(ref.shape), tuple(ref.stride()), ref.dtype, str(ref.device))
            zeros = _ZEROS.get(key)
            if zeros is None:
                zeros = torch.zeros_like(ref)
                if not torch.cuda.is_current_stream_capturing():   # (memory made inside a capture belongs to that graph's pool)
                    _ZEROS[key] = zeros
            a, b = (zeros if a is None else a), (zeros if b is None else b)
        # torch.cat keeps the memory format only when both halves already have it: checked BEFORE the launch, so that the result is
        # never thrown away for the copy path below
        if a.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format) and a.stride() == b.stride():
            out = torch.cat((a, b), dim=0)
            if out.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format):
                return out
    out = torch.empty((2 * n,) + tuple(ref.shape[1:]), dtype=ref.dtype, device=ref.device,
                      memory_format=torch.channels_last if cl else torch.contiguous_format)
    for half, t in ((out[:n], a), (out[n:], b)):
        if t is None:
            half.zero_()
        else:
            half.copy_(t)
    return out


_ZEROS = {}


def constants_snapshot():
    """The cached constants (zeros of _cat2) alive right now.  A captured graph that was recorded while they were cached replays
    reads of their memory: whoever owns the graph keeps this list for as long as the graph lives, and drop_constants() is then safe
    at any time."""
    return list(_ZEROS.values())


def drop_constants():
    """Forget the cached activation-sized constants (a new growing regime / batch size has other junction shapes; without this
    they pile up, one full-size tensor per shape ever seen)."""
    _ZEROS.clear()


class _CatBatch(Function):
    """Two activation batches as one (axis 0); the gradient comes back as the two contiguous halves.  Differentiable twice (the R1 penalty
    differentiates the first-order pass through the junction): the backward of the split is this concatenation again, an absent half
    being zeros.  Transparent to the premasked-gradient hand-off (see _premask_producer): when both halves are outputs of conv blocks with
    the same fused activation, the junction presents that activation to its consumer and passes the consumer's mark on to both producers
    -- the halves of an already masked gradient are already masked."""

    @staticmethod
    def forward(ctx, a, b, act, prods):
        ctx.set_materialize_grads(False)
        ctx._gs_act_out, ctx._prods, ctx._gs_premasked = act, prods, None
        return _cat2(a, b)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        masked = _take_premasked(ctx, g)
        if torch.is_grad_enabled():
            ga, gb = _SplitBatch.apply(g)
        else:
            n = g.shape[0] // 2
            ga, gb = g[:n], g[n:]
        if ctx._gs_act_out != ACT_NONE:   # (always rewritten: a mark left over from a pass that did not reach a producer must not survive)
            for prod, half in zip(ctx._prods, (ga, gb)):
                prod._gs_premasked = half.data_ptr() if masked else None
        return (ga if ctx.needs_input_grad[0] else None), (gb if ctx.needs_input_grad[1] else None), None, None


class _SplitBatch(Function):
    @staticmethod
    def forward(ctx, g):
        ctx.set_materialize_grads(False)
        n = g.shape[0] // 2
        return g[:n], g[n:]

    @staticmethod
    def backward(ctx, gga, ggb):
        if gga is None and ggb is None:
            return None
        return _cat2(gga, ggb)


def cat_batch(a, b):
    pa, pb = a.grad_fn, b.grad_fn
    act = getattr(pa, "_gs_act_out", ACT_NONE)
    if pa is None or pb is None or getattr(pb, "_gs_act_out", ACT_NONE) != act:
        act = ACT_NONE
    return _CatBatch.apply(a, b, act, (pa, pb))


def gan_d_loss(real_logits, fake_logits, labels, penalty, penalty_weight=1.0):
    """mean(softplus(-r) + softplus(f) + penalty_weight * penalty)."""
    return _GanDLoss.apply(real_logits, fake_logits, labels, penalty, float(penalty_weight))


def gan_g_loss(fake_logits, labels, sumsq, weight, eps):
    return _GanGLoss.apply(fake_logits, labels, sumsq, weight, eps)


# ----------------------------------------------------------------- R1 penalty reduction
class _SumSqRows(Function):
    """out[b] = sum_j x[b][...]^2  (models.py:48)."""

    @staticmethod
    def forward(ctx, x):
        if x.dim() == 2 and not x.is_contiguous():
            x = x.contiguous()   # (a column slice of a wider gradient: one copy serves this pass and the backward's row_scale)
        ctx.save_for_backward(x)
        return _K().sumsq_rows(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return _K().row_scale(x, g, 2.0)


def sumsq_rows(x):
    return _SumSqRows.apply(x)
