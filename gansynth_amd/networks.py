"""Progressive-GAN generator / discriminator on the HIP ops (reference networks.py:14-290).

Same constructor and call surface as the reference's PGGAN: `generator(latents, labels, name,
reuse)` -> images [B,2,128,1024]; `discriminator(images, labels, name, reuse)` -> (features,
logits).  The reference builds every tf.cond branch into one graph and lets the runtime pick;
here the growing depth is a host number, so each call walks the single active path: a trunk of
conv blocks below the current depth, then either the plain head or the faded (lerp) pair of
heads.  All variables of all depths are still created up front under the reference's scope
names, because the reference's graph owns them from step 0 (zero-gradient Adam updates included).
"""
import numpy as np
import torch

from . import config
from . import functional as F
from . import ops
from . import variables
from .variables import AUTO_REUSE, variable_scope


PIXEL_NORM_EPS = 1.0e-12   # ops.pixel_normalization default (ops.py:330)
_FUSE_NORM = not config.flag("GS_NO_FUSED_NORM")   # A/B switch for measurements


def _ilog2(ratio):
    ratio = np.asanyarray(ratio)
    depth = 0
    while not (ratio == 1).all():
        ratio = ratio >> 1
        depth += 1
    return depth


class PGGAN(object):

    def __init__(self, min_resolution, max_resolution, min_channels, max_channels, growing_level):
        self.min_resolution = np.asanyarray(min_resolution)
        self.max_resolution = np.asanyarray(max_resolution)
        self.min_channels = min_channels
        self.max_channels = max_channels
        self.growing_level = growing_level  # float, or a zero-argument callable (e.g. step / growing_steps)
        self.min_depth = 0
        self.fade_weight = None   # a functional.DeviceLerp: the trainer keeps the fade-in weight in device memory (hipGraph replay)
        self.max_depth = _ilog2(self.max_resolution // self.min_resolution)

    # ------------------------------------------------------------------ schedule (networks.py:24-29)
    @property
    def growing_depth(self):
        level = self.growing_level() if callable(self.growing_level) else self.growing_level
        full = np.float32((1 << (self.max_depth + 1)) - 1)
        return float(np.log2(np.float32(1.0) + full * np.float32(level)))

    def resolution(self, depth):
        return self.min_resolution << depth

    def channels(self, depth):
        return min(self.max_channels, self.min_channels << (self.max_depth - depth))

    def _block_name(self, kind, depth):
        return "{}_block_{}x{}".format(kind, *self.resolution(depth))

    def _head_depth(self, growing_depth):
        """Depth at which the recursion of networks.py:109-152 / 244-287 stops descending, and the
        lerp weight of the low-resolution branch there (None = plain head, no fade)."""
        depth = self.min_depth
        while depth < self.max_depth and growing_depth > depth:
            depth += 1
        if depth == self.min_depth and not growing_depth > depth:
            return depth, None
        if depth == self.max_depth and growing_depth > depth:
            return depth, None
        return depth, depth - growing_depth

    # ================================================================== generator
    def _g_conv_block(self, x, depth, sole_consumer=True):
        """`sole_consumer`: x (the previous block's normalised output) feeds nothing but this block -- false at the fade-in junction, where
        the low-resolution colour block reads it too (lets the backward fuse across the block boundary, ops.conv2d `input_normed`)."""
        c = self.channels(depth)
        with variable_scope(self._block_name("conv", depth)):
            if depth == self.min_depth:
                x = ops.pixel_normalization(x)
                with variable_scope("dense"):   # dense -> reshape -> leaky_relu (networks.py:43-55), then the norm
                    x = ops.dense_reshaped(x, c, self.resolution(depth), use_bias=True, variance_scale=2.0, scale_weight=True, activation="leaky_relu")
                    x = ops.pixel_normalization(x)
            else:
                with variable_scope("upscale_conv"):
                    x = ops.conv2d_transpose(x, filters=c, kernel_size=[3, 3], strides=[2, 2], use_bias=True,
                                             variance_scale=2.0, scale_weight=True, activation="leaky_relu",
                                             pixel_norm_epsilon=PIXEL_NORM_EPS if _FUSE_NORM else None,   # conv -> leaky_relu -> pixel norm: one node
                                             input_normed=sole_consumer)
                    if not _FUSE_NORM:
                        x = ops.pixel_normalization(x)
            with variable_scope("conv"):
                x = ops.conv2d(x, filters=c, kernel_size=[3, 3], use_bias=True, variance_scale=2.0, scale_weight=True,
                               activation="leaky_relu", pixel_norm_epsilon=PIXEL_NORM_EPS if _FUSE_NORM else None,
                               input_normed=depth != self.min_depth)   # (the upscale conv's output feeds this conv only)
                if not _FUSE_NORM:
                    x = ops.pixel_normalization(x)
        return x

    def _g_color_block(self, x, depth, sole_consumer=False):
        """`sole_consumer`: x (a conv block's normalised output) feeds nothing but this colour block (true for the head block's own output)."""
        with variable_scope(self._block_name("color", depth)):
            with variable_scope("conv"):
                return ops.conv2d(x, filters=2, kernel_size=[1, 1], use_bias=True, variance_scale=1.0, scale_weight=True,
                                  activation="tanh", input_normed=sole_consumer and _FUSE_NORM)

    def _g_variables(self, latent_dim, num_labels):
        """Create every generator variable (all depths) in the reference's scopes."""
        ops.get_weight([num_labels, latent_dim], 1.0, True)
        for depth in range(self.min_depth, self.max_depth + 1):
            c = self.channels(depth)
            with variable_scope(self._block_name("conv", depth)):
                if depth == self.min_depth:
                    with variable_scope("dense"):
                        units = c * int(self.resolution(depth).prod())
                        ops.get_weight([2 * latent_dim, units], 2.0, True)
                        ops.get_bias([units])
                else:
                    with variable_scope("upscale_conv"):
                        ops.get_weight([3, 3, self.channels(depth - 1), c], 2.0, True)
                        ops.get_bias([c])
                with variable_scope("conv"):
                    ops.get_weight([3, 3, c, c], 2.0, True)
                    ops.get_bias([c])
            with variable_scope(self._block_name("color", depth)):
                with variable_scope("conv"):
                    ops.get_weight([1, 1, c, 2], 1.0, True)
                    ops.get_bias([2])

    def generator(self, latents, labels, name="generator", reuse=AUTO_REUSE):
        F.tap_begin("generator")
        with variable_scope(name, reuse=reuse):
            self._g_variables(latents.shape[1], labels.shape[1])
            embedded = ops.embedding(labels, units=latents.shape[1], variance_scale=1.0, scale_weight=True)
            x = torch.cat([latents, embedded], dim=1)
            head, fade = self._head_depth(self.growing_depth)
            for depth in range(self.min_depth, head):
                x = self._g_conv_block(x, depth)
            full = self.resolution(self.max_depth)
            middle = ops.upscale2d(self._g_color_block(self._g_conv_block(x, head, sole_consumer=fade is None), head, sole_consumer=True), full // self.resolution(head))
            if fade is None:
                return middle
            low = ops.upscale2d(self._g_color_block(x, head - 1), full // self.resolution(head - 1))
            return ops.lerp(low, middle, fade if self.fade_weight is None else self.fade_weight)

    # ============================================================== discriminator
    def _d_conv_block(self, x, depth, num_labels, fresh_activation=False, sub_batches=1):
        """`fresh_activation`: x is the leaky-relu output of the previous conv and feeds nothing but this block's first conv
        (true along the trunk, false after the fade-in lerp) -- lets the backward fold the activation derivative into the
        data-gradient kernel (ops.conv2d `input_activation`)."""
        c = self.channels(depth)
        with variable_scope(self._block_name("conv", depth)):
            if depth == self.min_depth:
                # networks.py:174-184: conv(concat([x, batch_stddev(x)])).  The 257-channel conv is
                # evaluated as conv(x; w[:,:,:c]) + conv(stddev; w[:,:,c:]) -- same variable, same
                # fan-in scale, no 257-wide tensor (257 is not an MFMA-friendly K).
                x, stddev = ops.batch_stddev_tap(x, sub_batches=sub_batches)   # (x through the tap: one consumer, the two gradients summed in one kernel)
                with variable_scope("conv"):
                    weight, alpha = ops.get_weight([3, 3, c + 1, c], 2.0, True)
                    bias = ops.get_bias([c])
                    y = F.axpby(F.conv2d(x, F.weight_slice(weight, 0, c), 3, 1, alpha),
                                F.conv2d(stddev, F.weight_slice(weight, c, c + 1), 3, 1, alpha), 1.0, 1.0)
                    x = F.bias_act(y, bias, ops._ACT["leaky_relu"])
                with variable_scope("dense"):
                    # tf.layers.flatten of NCHW (channel-major) happens inside ops.dense (4-D input)
                    features = ops.dense(x, units=self.channels(depth - 1), use_bias=True, variance_scale=2.0,
                                         scale_weight=True, activation="leaky_relu")
                with variable_scope("logits"):
                    logits = ops.dense(features, units=num_labels, use_bias=True, variance_scale=1.0, scale_weight=True)
                return features, logits
            with variable_scope("conv"):
                x = ops.conv2d(x, filters=c, kernel_size=[3, 3], use_bias=True, variance_scale=2.0, scale_weight=True,
                               activation="leaky_relu", input_activation="leaky_relu" if fresh_activation else None)
            with variable_scope("conv_downscale"):
                x = ops.conv2d(x, filters=self.channels(depth - 1), kernel_size=[3, 3], strides=[2, 2], use_bias=True,
                               variance_scale=2.0, scale_weight=True, activation="leaky_relu", input_activation="leaky_relu")
            return x

    def _d_color_block(self, x, depth):
        with variable_scope(self._block_name("color", depth)):
            with variable_scope("conv"):
                return ops.conv2d(x, filters=self.channels(depth), kernel_size=[1, 1], use_bias=True, variance_scale=2.0,
                                  scale_weight=True, activation="leaky_relu")

    def _d_variables(self, num_labels):
        for depth in range(self.min_depth, self.max_depth + 1):
            c = self.channels(depth)
            with variable_scope(self._block_name("color", depth)):
                with variable_scope("conv"):
                    ops.get_weight([1, 1, 2, c], 2.0, True)
                    ops.get_bias([c])
            with variable_scope(self._block_name("conv", depth)):
                if depth == self.min_depth:
                    with variable_scope("conv"):
                        ops.get_weight([3, 3, c + 1, c], 2.0, True)
                        ops.get_bias([c])
                    with variable_scope("dense"):
                        ops.get_weight([c * int(self.resolution(depth).prod()), self.channels(depth - 1)], 2.0, True)
                        ops.get_bias([self.channels(depth - 1)])
                    with variable_scope("logits"):
                        ops.get_weight([self.channels(depth - 1), num_labels], 1.0, True)
                        ops.get_bias([num_labels])
                else:
                    with variable_scope("conv"):
                        ops.get_weight([3, 3, c, c], 2.0, True)
                        ops.get_bias([c])
                    with variable_scope("conv_downscale"):
                        ops.get_weight([3, 3, c, self.channels(depth - 1)], 2.0, True)
                        ops.get_bias([self.channels(depth - 1)])

    # The discriminator in two pieces (same variables, same launches as `discriminator`):
    #   trunk: colour block(s), the head block, the fade-in junction and the blocks down to `tail_top`
    #   tail:  the blocks from `tail_top` (at most 8x64) down to the 2x16 block with its statistic, dense and logits
    # Every launch of the tail is latency-bound at batch 8 (a few tens of blocks on 256 CUs), so the trainer runs the tails of the real and
    # of the fake pass of a discriminator run as ONE pass over the concatenated batch (models.GANSynth._d_losses_b): `sub_batches` keeps
    # the minibatch statistic per original batch (ops.py:336-348 on each half).
    TAIL_LEVELS = int(config.value("GS_D_TAIL_LEVELS", "3"))   # (measured: see DESIGN.md 6.3)

    def _tail_top(self, head):
        return max(self.min_depth, min(head - 1, self.min_depth + self.TAIL_LEVELS - 1))

    def discriminator_trunk(self, images, num_labels, name="discriminator", reuse=AUTO_REUSE):
        """-> (x, depth, fresh): the input of block `depth` (the first block of the tail)."""
        F.tap_begin("discriminator")
        with variable_scope(name, reuse=reuse):
            self._d_variables(num_labels)
            head, fade = self._head_depth(self.growing_depth)
            full = self.resolution(self.max_depth)

            def from_images(depth):
                return self._d_color_block(ops.downscale2d(images, full // self.resolution(depth)), depth)

            if head == self.min_depth:
                return from_images(head), head, False
            low = from_images(head - 1) if fade is not None else None   # lerp(low(), middle(), .): low first, like networks.py:271-275
            x = self._d_conv_block(from_images(head), head, num_labels, fresh_activation=True)
            fresh = fade is None
            if fade is not None:
                x = ops.lerp(low, x, fade if self.fade_weight is None else self.fade_weight)
            top = self._tail_top(head)
            for depth in range(head - 1, top, -1):
                x = self._d_conv_block(x, depth, num_labels, fresh_activation=fresh)
                fresh = True
            return x, top, fresh

    def discriminator_tail(self, x, depth, fresh, labels, sub_batches=1, name="discriminator", reuse=AUTO_REUSE):
        num_labels = labels.shape[1]
        with variable_scope(name, reuse=reuse):
            self._d_variables(num_labels)
            for d in range(depth, self.min_depth, -1):
                x = self._d_conv_block(x, d, num_labels, fresh_activation=fresh)
                fresh = True
            # (x also feeds batch_stddev in the last block: never fused)
            return self._d_conv_block(x, self.min_depth, num_labels, fresh_activation=False, sub_batches=sub_batches)

    def discriminator(self, images, labels, name="discriminator", reuse=AUTO_REUSE):
        x, depth, fresh = self.discriminator_trunk(images, labels.shape[1], name=name, reuse=reuse)
        return self.discriminator_tail(x, depth, fresh, labels, name=name, reuse=reuse)


# ====================================================================================================== pitch classifier
GN_EPS = 1.0e-12   # ops.group_normalization / ops.weight_standardization default (ops.py:53,120)


class ResNet(object):
    """The pitch classifier of networks.py:293-413: GANSynth.evaluate's feature extractor (`__call__`, inference) and its training pass
    (`forward_backward` / `momentum_step`, fp32).

    Same constructor and call surface: `resnet(images, name="resnet", reuse)` -> (features [n, filters of the last stage] fp32,
    logits [n, classes] fp32); images [n, 2, 128, 1024] (channels-last, fp32 or bf16: the activation dtype of the whole pass).
    Variables use the reference's scope names and layouts ("resnet/conv/weight" [7, 7, 2, 64], "resnet/residual_block_0_0/
    group_normalization_1st/gamma" [1, 64, 1, 1], "resnet/logits/weight" [512, 61], ...) and live in the classifier's OWN store, so a
    GAN's parameters, checkpoints and graphs never see them.  Every conv is weight-standardised (ops.py:53-66): the standardised copy of
    a weight is computed once per weight value (re-done when the variable changes) and the convs run on it with alpha = 1.
    Per block (pre-activation, networks.py:306-353): GN -> ReLU (one pass, the statistics already known), [1x1 projection], 3x3 conv
    + bias, GN statistics, GN -> ReLU, 3x3 conv + bias, then the residual add inside the pass that takes the NEXT normalisation's
    statistics (the sum is stored once there: it is the next block's input and shortcut).  The stem conv and the max pool are one
    kernel; the head (GN -> ReLU -> mean over H, W) is one kernel."""

    def __init__(self, conv_param, pool_param, residual_params, groups, classes, store=None):
        self.conv_param = conv_param
        self.pool_param = pool_param
        self.residual_params = residual_params
        self.groups = groups
        self.classes = classes
        if store is None:
            store = variables.VariableStore(device="cuda" if torch.cuda.is_available() else "cpu", seed=0)
        self.store = store
        self._prep = {}   # variable name -> [stamp, standardised weight, {dtype: [conv workspace, prepared]}]
        self._train = None   # train_state()

    @staticmethod
    def pitch_classifier(store=None):
        """pitch_classifier_main.py:39-50."""
        from .utils import Dict
        return ResNet(conv_param=Dict(filters=64, kernel_size=[7, 7], strides=[2, 2]),
                      pool_param=Dict(kernel_size=[3, 3], strides=[2, 2]),
                      residual_params=[Dict(filters=64, strides=[1, 1], blocks=3), Dict(filters=128, strides=[2, 2], blocks=4),
                                       Dict(filters=256, strides=[2, 2], blocks=6), Dict(filters=512, strides=[2, 2], blocks=3)],
                      groups=32, classes=len(range(24, 85)), store=store)

    # ------------------------------------------------------------------------------------------------- variables
    def _conv_vars(self, ksize, ci, co, use_bias):
        """ops.get_weight / get_bias of conv2d(variance_scale=2.0) (ops.py:149-180, 221-229)."""
        stddev = float(np.sqrt(2.0 / (ksize * ksize * ci)))
        w = self.store.get_variable("weight", [ksize, ksize, ci, co], variables.truncated_normal(0.0, stddev))
        b = self.store.get_variable("bias", [co], variables.zeros()) if use_bias else None
        return w, b

    def _gn_vars(self, c):
        """ops.py:136-145 (beta first, then gamma)."""
        beta = self.store.get_variable("beta", [1, c, 1, 1], variables.zeros())
        gamma = self.store.get_variable("gamma", [1, c, 1, 1], variables.ones())
        return beta, gamma

    def create_variables(self, in_channels=2, name="resnet"):
        """Every variable of the network, in the reference's creation order, without running anything."""
        self._walk(None, in_channels, name)
        return self.store.variables

    def load_state_dict(self, state, strict=True):
        """{variable name: array} -> the store; a missing variable or a wrong shape is refused by name."""
        if not self.store.variables:
            self.create_variables()
        for k, v in self.store.variables.items():
            if k not in state:
                raise KeyError(f"classifier weights lack the variable {k} {tuple(v.shape)}")
            if tuple(np.shape(state[k])) != tuple(v.shape):
                raise ValueError(f"classifier variable {k} has shape {tuple(np.shape(state[k]))}, the network needs {tuple(v.shape)}")
        if strict:
            extra = [k for k in state if k not in self.store.variables and k.startswith("resnet/")]
            if extra:
                raise KeyError(f"classifier weights hold variables the network does not have: {extra[:4]}")
        with torch.no_grad():
            for k, v in self.store.variables.items():
                v.copy_(torch.as_tensor(np.asarray(state[k], dtype=np.float32)).to(v.device))
        self._prep.clear()

    def load(self, source):
        """A frozen GraphDef (.pb path or bytes) or a .safetensors file under the reference's variable names."""
        from . import classifier_io
        self.load_state_dict(classifier_io.load_classifier_weights(source, names=list(self.create_variables()) if not self.store.variables
                                                                   else list(self.store.variables)))
        return self

    # ---------------------------------------------------------------------------------------------- prepared weights
    def _standardized(self, w):
        """The weight-standardised copy of variable w (fp32, same layout), recomputed only when w changes."""
        key = id(w)
        stamp = (w.data_ptr(), w._version)
        ent = self._prep.get(key)
        if ent is None or ent[0] != stamp:
            from . import kernels
            std = kernels.get().weight_standardize(w.detach(), GN_EPS, out=None if ent is None else ent[1])
            ent = [stamp, std, {}]
            self._prep[key] = ent
        return ent

    def _conv3x3(self, x, w, b, stride):
        from . import kernels
        K = kernels.get()
        ent = self._standardized(w)
        dt = kernels._dt(x)
        slot = ent[2].get(dt)
        if slot is None:
            slot = ent[2][dt] = [K.conv2d_fwd_workspace(tuple(x.shape), w.shape[3], 3, stride, dt), 0]
        y = K.conv2d_fwd_bias_ws(x, ent[1], b, 3, stride, slot[0], slot[1])
        slot[1] = 1
        return y

    # --------------------------------------------------------------------------------------------------- training
    # A hand-scheduled reverse walk instead of autograd Functions: the step is one fixed sequence of launches (nothing to trace, no
    # graph of Python objects per step), every saved tensor is named here, the gradients land in the flat buffer's views directly,
    # and the fusions the backward wants (the shortcut gradient as the norm backward's addend, the projection's data gradient added
    # into the conv's) cross what would be node boundaries.
    @staticmethod
    def is_decayed(name):
        """models.py:268-272: the L2 term covers every trainable variable whose name does not contain "normalization"."""
        return "normalization" not in name

    def train_state(self, name="resnet"):
        """The training-side storage, built on first use: every variable re-homed into one flat fp32 buffer (flat_params._FlatParams:
        .flat, .grad, .m = the momentum accumulators) with the decayed variables first -- one contiguous decayed range --, the
        standardised copies of the conv weights and their gradients in flat buffers of their own, and the descriptor table of the
        batched standardisation."""
        if getattr(self, "_train", None) is not None:
            return self._train
        from . import kernels
        from .flat_params import _FlatParams
        from .utils import Dict
        if not self.store.variables:
            self.create_variables(name=name)
        V = self.store.variables
        order = [k for k in V if self.is_decayed(k)] + [k for k in V if not self.is_decayed(k)]
        flat = _FlatParams([(k, V[k]) for k in order])
        flat.v = None   # (Adam's second slot: momentum has one)
        decay_hi = next((off for off, _, k in flat._offsets if not self.is_decayed(k)), flat.flat.numel())
        convs = [k for k in order if k.endswith("/weight") and V[k].dim() == 4]
        pad = lambda n: (n + 63) // 64 * 64
        total, chans = sum(pad(V[k].numel()) for k in convs), sum(pad(V[k].shape[3]) for k in convs)
        dev = flat.flat.device
        std, gstd, rstd = (torch.zeros(n, dtype=torch.float32, device=dev) for n in (total, total, chans))
        views, rows, o, oc = {}, [], 0, 0
        for k in convs:
            w = V[k]
            n, co = w.numel(), w.shape[3]
            views[k] = (std[o:o + n].view(w.shape), gstd[o:o + n].view(w.shape))
            rows.append((w.data, views[k][0], rstd[oc:oc + co], views[k][1], w.grad))
            o, oc = o + pad(n), oc + pad(co)
        # gstd_clean: the standardised weights' gradient buffer is all zeros (fresh, or cleared by the last pass's final launch)
        self._train = Dict(flat=flat, decay_range=(0, decay_hi), std=views, gstd=gstd, gstd_clean=True, table=kernels.get().weight_standardize_table(rows), ws={}, name=name)
        self._prep.clear()   # (the variables moved)
        return self._train

    def parameters_changed(self):
        """The variables were updated in place by a kernel (no torch version bump): the inference path's standardised copies are stale."""
        for ent in self._prep.values():
            ent[0] = None

    def _conv3x3_train(self, K, st, x, key, stride):
        V = self.store.variables
        w = st.std[key + "/weight"][0]
        from . import kernels
        wk = (key, tuple(x.shape))
        if wk not in st.ws:
            st.ws[wk] = K.conv2d_fwd_workspace(tuple(x.shape), w.shape[3], 3, stride, kernels._dt(x))
        return K.conv2d_fwd_bias_ws(x, w, V[key + "/bias"].data, 3, stride, st.ws[wk], 0)

    def forward_backward(self, images, onehot_labels, name="resnet"):
        """One training pass: -> (loss_xent [1] fp32 = the mean softmax cross-entropy WITHOUT the L2 term, correct [1] int32 = rows whose
        argmax is the label's, features, logits), and the gradient of that loss w.r.t. every variable in the flat gradient buffer
        (train_state().flat.grad; each variable's .grad is its view).  The L2 term's gradient, weight_decay * v, is added by the
        optimizer step (kernels.momentum_tf_step).  fp32 activations; the images receive no gradient."""
        from . import kernels
        from ._lib import ACT_NONE
        if images.dtype != torch.float32:
            raise TypeError(f"ResNet.forward_backward: activations are {images.dtype}; training runs in fp32 (bf16 training is not implemented)")
        K = kernels.get()
        st = self.train_state(name)
        if st.name != name:
            raise ValueError(f"ResNet.forward_backward: the training state was built under the scope {st.name!r}")
        V, G = self.store.variables, self.groups
        S = lambda key: st.std[key + "/weight"]          # (standardised weight, its gradient buffer)
        gn = lambda key: (V[key + "/gamma"].data.view(-1), V[key + "/beta"].data.view(-1))
        gn_grads = lambda key: dict(dgamma=V[key + "/gamma"].grad.view(-1), dbeta=V[key + "/beta"].grad.view(-1))
        with torch.no_grad():
            st.flat.begin_run()
            if not st.gstd_clean:   # the previous pass raised before its last launch: its partial sums must not be added onto
                st.gstd.zero_()
            st.gstd_clean = False
            K.weight_standardize_batch(st.table, GN_EPS)
            images = images.contiguous(memory_format=torch.channels_last)
            labels = onehot_labels.to(device=images.device, dtype=torch.float32)
            # ---- forward, keeping what the backward reads
            stem, x = K.resnet_stem_pool(images, S(name + "/conv")[0], V[name + "/conv/bias"].data, want_stem=True)
            stats, _ = K.group_norm_stats(x, G, GN_EPS)
            tape = []
            for i, rp in enumerate(self.residual_params):
                for j in range(rp.blocks):
                    stride = int(rp.strides[0]) if j == 0 else 1
                    b = f"{name}/residual_block_{i}_{j}"
                    x_in, st1 = x, stats
                    a = K.group_norm_apply(x, stats, *gn(b + "/group_normalization_1st"), relu=True)
                    shortcut = K.conv1x1_fwd(a, S(b + "/projection_shortcut")[0], stride) if j == 0 else x
                    t1 = self._conv3x3_train(K, st, a, b + "/conv_1st", stride)
                    st2, _ = K.group_norm_stats(t1, G, GN_EPS)
                    a2 = K.group_norm_apply(t1, st2, *gn(b + "/group_normalization_2nd"), relu=True)
                    t2 = self._conv3x3_train(K, st, a2, b + "/conv_2nd", 1)
                    stats, x = K.group_norm_stats(t2, G, GN_EPS, addend=shortcut)
                    tape.append((b, j == 0, stride, x_in, st1, a, t1, st2, a2))
            features = K.group_norm_relu_mean(x, stats, *gn(name + "/group_normalization"))
            wl, bl = V[name + "/logits/weight"], V[name + "/logits/bias"]
            logits = torch.cat([K.dense_fwd_bias_act(features[r:r + 64], wl.data, bl.data, 1.0, ACT_NONE) for r in range(0, features.shape[0], 64)])
            loss, dlogits, correct = K.softmax_xent(logits, labels)
            # ---- backward
            K.dense_bwd_weight(features, dlogits, 1.0, out=wl.grad)
            K.channel_sum(dlogits, out=bl.grad)
            dfeat = K.dense_bwd_data(dlogits, wl.data, 1.0)
            dx, _, _ = K.group_norm_relu_mean_bwd(x, stats, *gn(name + "/group_normalization"), dfeat, **gn_grads(name + "/group_normalization"))
            for b, projected, stride, x_in, st1, a, t1, st2, a2 in reversed(tape):
                w2, gw2 = S(b + "/conv_2nd")
                K.conv2d_bwd_weight(a2, dx, 3, 1, 1.0, out=gw2, bias_out=V[b + "/conv_2nd/bias"].grad)
                da2 = K.conv2d_bwd_data(dx, w2, tuple(a2.shape), 3, 1, 1.0)
                dt1, _, _ = K.group_norm_relu_bwd(t1, st2, *gn(b + "/group_normalization_2nd"), da2, **gn_grads(b + "/group_normalization_2nd"))
                w1, gw1 = S(b + "/conv_1st")
                K.conv2d_bwd_weight(a, dt1, 3, stride, 1.0, out=gw1, bias_out=V[b + "/conv_1st/bias"].grad)
                da = K.conv2d_bwd_data(dt1, w1, tuple(a.shape), 3, stride, 1.0)
                addend = dx   # the identity shortcut's gradient joins inside the norm's backward
                if projected:
                    wp, gwp = S(b + "/projection_shortcut")
                    K.conv1x1_bwd_weight(a, dx, stride, out=gwp)
                    K.conv1x1_bwd_data(dx, wp, tuple(a.shape), stride, out=da)
                    addend = None
                dx, _, _ = K.group_norm_relu_bwd(x_in, st1, *gn(b + "/group_normalization_1st"), da, addend=addend,
                                                 **gn_grads(b + "/group_normalization_1st"))
            dstem = K.max_pool2d_bwd(stem, dx)
            K.resnet_stem_bwd_weight(images, dstem, out=S(name + "/conv")[1], bias_out=V[name + "/conv/bias"].grad)
            K.weight_standardize_bwd_batch(st.table)   # d standardised weights -> the variables' gradients (and cleared for the next pass)
            st.gstd_clean = True
        return loss, correct, features, logits

    def momentum_step(self, lr, momentum, use_nesterov, weight_decay):
        """tf.train.MomentumOptimizer.apply_gradients on the flat buffer, the L2 term's gradient folded in (one launch; the gradient
        buffer is cleared behind it).  Returns sum v^2 / 2 over the decayed variables at the pre-update values ([1] fp32)."""
        from . import kernels
        st = self.train_state()
        l2 = kernels.get().momentum_tf_step(st.flat.flat, st.flat.grad, st.flat.m, lr, momentum, use_nesterov, weight_decay=weight_decay,
                                            decay_range=st.decay_range, zero_grad=True, want_l2=True)
        st.flat.grad_clean = True
        st.flat.t += 1
        self.parameters_changed()
        return l2

    # --------------------------------------------------------------------------------------------------- forward
    def __call__(self, inputs, name="resnet", reuse=AUTO_REUSE):
        with torch.no_grad():
            return self._walk(inputs, inputs.shape[1], name)

    def _walk(self, x, in_channels, name):
        """The forward of networks.py:355-413 (x None: create the variables only)."""
        from . import kernels
        K = kernels.get() if x is not None else None
        scope = self.store.variable_scope
        cp, pp, G = self.conv_param, self.pool_param, self.groups
        if not (cp and list(cp.kernel_size) == [7, 7] and list(cp.strides) == [2, 2] and pp and list(pp.kernel_size) == [3, 3]
                and list(pp.strides) == [2, 2] and cp.filters == 64 and in_channels == 2):
            raise ValueError("ResNet: the stem is the pitch classifier's (conv 7x7 / 2, 2 -> 64 channels, max pool 3x3 / 2: "
                             "pitch_classifier_main.py:39-41)")
        with scope(name):
            with scope("conv"):
                w, b = self._conv_vars(7, in_channels, cp.filters, True)
            stats = None
            if x is not None:
                _, x = K.resnet_stem_pool(x, self._standardized(w)[1], b)
                stats, _ = K.group_norm_stats(x, G, GN_EPS)
            c = cp.filters
            for i, rp in enumerate(self.residual_params):
                for j in range(rp.blocks):
                    stride = int(rp.strides[0]) if j == 0 else 1
                    if list(rp.strides) not in ([1, 1], [2, 2]):
                        raise ValueError(f"ResNet: residual strides {rp.strides}")
                    with scope(f"residual_block_{i}_{j}"):
                        with scope("group_normalization_1st"):
                            beta, gamma = self._gn_vars(c)
                        shortcut = x
                        if x is not None:
                            x = K.group_norm_apply(x, stats, gamma, beta, relu=True)
                        if j == 0:   # projection_shortcut=True for the first block of every stage (networks.py:370-378)
                            with scope("projection_shortcut"):
                                wp, _ = self._conv_vars(1, c, rp.filters, False)
                            if x is not None:
                                shortcut = K.conv1x1_fwd(x, self._standardized(wp)[1], stride)
                        with scope("conv_1st"):
                            w1, b1 = self._conv_vars(3, c, rp.filters, True)
                        with scope("group_normalization_2nd"):
                            beta2, gamma2 = self._gn_vars(rp.filters)
                        with scope("conv_2nd"):
                            w2, b2 = self._conv_vars(3, rp.filters, rp.filters, True)
                        if x is not None:
                            t = self._conv3x3(x, w1, b1, stride)
                            st2, _ = K.group_norm_stats(t, G, GN_EPS)
                            t = K.group_norm_apply(t, st2, gamma2, beta2, relu=True)
                            t = self._conv3x3(t, w2, b2, 1)
                            stats, x = K.group_norm_stats(t, G, GN_EPS, addend=shortcut)   # inputs += shortcut, stored once
                    c = rp.filters
            with scope("group_normalization"):
                beta, gamma = self._gn_vars(c)
            features = K.group_norm_relu_mean(x, stats, gamma, beta) if x is not None else None
            with scope("logits"):   # dense(variance_scale=1.0), no weight standardisation (networks.py:404-411)
                wl = self.store.get_variable("weight", [c, self.classes], variables.truncated_normal(0.0, float(np.sqrt(1.0 / c))))
                bl = self.store.get_variable("bias", [self.classes], variables.zeros())
            if x is None:
                return None
            from ._lib import ACT_NONE
            # (the small-batch dense kernel: 64 rows per launch)
            logits = torch.cat([K.dense_fwd_bias_act(features[r:r + 64], wl, bl, 1.0, ACT_NONE) for r in range(0, features.shape[0], 64)])
            return features, logits
