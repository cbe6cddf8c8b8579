"""Convolution modules whose arithmetic runs in libpwgkernels.so.

They replace ``torch.nn.Conv1d`` / ``torch.nn.ConvTranspose1d`` / ``torch.nn.Conv2d`` with
``(k, 1)`` kernels, together with the old-style ``torch.nn.utils.weight_norm`` /
``spectral_norm`` hooks, at the reference's call sites.  Parameter and buffer names and shapes
are the reference's, so its checkpoints load unchanged:
``weight``/``bias``; with weight norm ``weight_g``/``weight_v``/``bias``; with spectral norm
``weight_orig``/``weight_u``/``weight_v``/``bias``
(e.g. /root/reference/parallel_wavegan/models/hifigan.py:221-231, :383-402, :603-621).

Inference (no grad): the packed kernel weight image is derived once on the device and cached
until a parameter changes.  Training: the effective weight is a differentiable HIP node
(functional.WeightNormFn / SpectralNormFn) feeding functional.FusedConvFn.
"""
import math
import os

import torch

from .. import functional as Fn
from .. import ops


class _ConvNd(torch.nn.Module):
    transposed = False
    width_mode = False  # True for the (k, 1) Conv2d: input is (B, C, H, W)
    explicit_pad_min_elems = 1 << 20  # no-grad forward with reflect / replicate padding: see forward()
    # Batch folding (forward() / _fold_batch): on by default (C3 49.36 -> 48.29 ms, C5 45.52 -> 44.29 ms per captured
    # step, C4 / C2 unchanged; 64 or 128 columns per item measured slower: profiles/r05_fold_batch_ab.txt);
    # PWG_FOLD_BATCH=0 switches it off for A/B runs
    fold_batch = {"0": False, "1": True}.get(os.environ.get("PWG_FOLD_BATCH", ""), True)
    fold_max_cols = int(os.environ.get("PWG_FOLD_MAX_COLS", 40))  # output columns per item up to which a layer is folded
    fold_min_weight_bytes = 4 << 20  # ... if its weight is at least this large (the launch streams it once per item)
    # Inference precision of this module: "fp32" (default) or "bf16" -- bf16 OPERANDS on the bf16 MFMA kernel
    # (csrc/conv1d_bf16.hip), fp32 accumulation, epilogue and tensors; inference only.  Set through
    # utils.set_inference_precision; a layer the bf16 kernel does not cover stays on the fp32 kernels.
    precision = "fp32"
    # Split-operand fp32 inference (csrc/conv1d_split.hip): a no-grad forward of an fp32 module whose
    # class is in SPLIT_ADMITTED runs on the bf16 MFMA with 3-way split operands.  On by default; PWG_SPLIT_EXACT=0
    # switches it off for A/B runs (read once).  split_admit_all (tests, measurements): every layer the kernel supports.
    split_exact = {"0": False, "1": True}.get(os.environ.get("PWG_SPLIT_EXACT", ""), True)
    split_admit_all = False

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 bias=True, output_padding=0, pad_mode="zero"):
        super().__init__()
        if in_channels % groups or out_channels % groups:
            raise ValueError("in_channels and out_channels must be divisible by groups")
        self.in_channels, self.out_channels = in_channels, out_channels
        # padding: int (both sides) or (left, right) -- causal layers pad on the left only
        if isinstance(padding, (tuple, list)):
            padding, self.padding_right = int(padding[0]), int(padding[1])
        else:
            self.padding_right = int(padding)
        self.kernel_size, self.stride, self.padding = int(kernel_size), int(stride), int(padding)
        self.dilation, self.groups, self.output_padding = int(dilation), int(groups), int(output_padding)
        self.pad_mode = pad_mode
        self.weight = torch.nn.Parameter(torch.empty(self._weight_shape()))
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self._cache_packed = None  # functional.PreparedWeights; current while its key equals _params_key()
        self.spectral_eps = 1e-12
        self.reset_parameters()

    def _weight_shape(self):
        if self.transposed:
            return (self.in_channels, self.out_channels // self.groups, self.kernel_size)
        return (self.out_channels, self.in_channels // self.groups, self.kernel_size)

    # -- initialisation identical in distribution to torch.nn.Conv1d's default
    def reset_parameters(self):
        w = self.raw_weight
        fan_in = int(w[0].numel())
        bound = 1.0 / math.sqrt(fan_in) if fan_in > 0 else 0.0
        with torch.no_grad():
            w.uniform_(-bound, bound)  # kaiming_uniform_(a=sqrt(5)) == U(-1/sqrt(fan_in), 1/sqrt(fan_in))
            if self.bias is not None:
                self.bias.uniform_(-bound, bound)

    @property
    def raw_weight(self):
        """The directly trainable weight-shaped parameter (weight / weight_v / weight_orig)."""
        if self.has_weight_norm:
            return self.weight_v
        if self.has_spectral_norm:
            return self.weight_orig
        return self.weight

    # -- old-style weight norm (dim=0): w = g * v / ||v||
    @property
    def has_weight_norm(self):
        return "weight_g" in self._parameters

    @property
    def has_spectral_norm(self):
        return "weight_orig" in self._parameters

    def apply_weight_norm(self):
        if self.has_weight_norm:
            return self
        if self.has_spectral_norm:
            raise ValueError("spectral norm is already applied")
        w = self._parameters.pop("weight")
        with torch.no_grad():
            g = w.detach().reshape(w.shape[0], -1).norm(dim=1).reshape((-1,) + (1,) * (w.dim() - 1))
        self.weight_g = torch.nn.Parameter(g.clone())
        self.weight_v = torch.nn.Parameter(w.detach().clone())
        self._cache_packed = None
        return self

    def remove_weight_norm(self):
        if not self.has_weight_norm:
            raise ValueError(f"weight norm is not applied to {self.__class__.__name__}")
        g, v = self._parameters.pop("weight_g"), self._parameters.pop("weight_v")
        self.weight = torch.nn.Parameter(self._bake_weight_norm(g.detach(), v.detach()))
        self._cache_packed = None
        return self

    @staticmethod
    def _bake_weight_norm(g, v):
        """One-off parameter conversion for ``remove_weight_norm`` (checkpoint bookkeeping; the
        reference calls it on CPU before ``.to(device)``, bin/decode.py:147-149).  On the device
        it runs on the HIP kernels; on the host it is plain parameter arithmetic, never a
        substitute for the compute path."""
        if v.is_cuda:
            vc = v.contiguous()
            return ops.scale_rows(vc, ops.weight_norm_scale(vc, g.reshape(-1).contiguous()))
        n = v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape)
        return v * (g / n)

    # -- old-style spectral norm (dim=0, one power iteration per training forward)
    def apply_spectral_norm(self):
        if self.has_spectral_norm:
            return self
        if self.has_weight_norm:
            raise ValueError("weight norm is already applied")
        w = self._parameters.pop("weight")
        rows, cols = w.shape[0], w[0].numel()
        with torch.no_grad():
            # torch.nn.utils.spectral_norm: u ~ N(0,1) normalised, v likewise, then 15 warm-up
            # iterations at construction time (host-side initialisation only)
            u = torch.nn.functional.normalize(torch.randn(rows), dim=0, eps=self.spectral_eps)
            v = torch.nn.functional.normalize(torch.randn(cols), dim=0, eps=self.spectral_eps)
            wm = w.detach().reshape(rows, cols)
            for _ in range(15):
                v = torch.nn.functional.normalize(torch.mv(wm.t(), u), dim=0, eps=self.spectral_eps)
                u = torch.nn.functional.normalize(torch.mv(wm, v), dim=0, eps=self.spectral_eps)
        self.weight_orig = torch.nn.Parameter(w.detach().clone())
        self.register_buffer("weight_u", u)
        self.register_buffer("weight_v", v)
        self._cache_packed = None
        return self

    def remove_spectral_norm(self):
        if not self.has_spectral_norm:
            raise ValueError(f"spectral norm is not applied to {self.__class__.__name__}")
        w = self._parameters.pop("weight_orig")
        u, v = self._buffers.pop("weight_u"), self._buffers.pop("weight_v")
        with torch.no_grad():
            wm = w.detach().reshape(w.shape[0], -1)
            sigma = torch.dot(u, torch.mv(wm, v))
        self.weight = torch.nn.Parameter(w.detach() / sigma)
        self._cache_packed = None
        return self

    # -- effective weight
    def weight_tensor(self):
        """Differentiable effective weight (torch layout) computed by HIP kernels."""
        if self.has_weight_norm:
            return Fn.WeightNormFn.apply(self.weight_v, self.weight_g)
        if self.has_spectral_norm:
            return Fn.SpectralNormFn.apply(self.weight_orig, self.weight_u, self.weight_v, self.training,
                                           self.spectral_eps)
        return self.weight

    def effective_weight(self):
        with torch.no_grad():
            return self.weight_tensor().detach()

    def _param_state(self):
        """``ops.tensor_state`` of the tensors the effective weight is derived from (the key without the global epoch)."""
        ps = [self.raw_weight] + ([self.weight_g] if self.has_weight_norm else [])
        if self.has_spectral_norm:
            ps += [self.weight_u, self.weight_v]
        return tuple(ops.tensor_state(p) for p in ps)

    def _params_key(self):
        """The key every image derived from this layer's weight is cached under."""
        return (ops.cache_epoch(),) + self._param_state()

    def prepared(self):
        """:class:`functional.PreparedWeights` for the current parameter values (weight or weight-norm
        layers): weight-norm scale, packed forward image and, lazily, the packed data-gradient image.
        Shared by every forward / backward until a parameter changes."""
        key = self._params_key()
        if self._cache_packed is None or self._cache_packed.key != key:
            desc = self.make_desc(1, self._probe_len())
            with torch.no_grad():
                if self.has_weight_norm:
                    v = self._w3(self.weight_v.detach())
                    scale = ops.weight_norm_scale(v, self.weight_g.detach().reshape(-1).contiguous())
                    self._cache_packed = Fn.PreparedWeights(key, v, scale, None, desc)
                else:
                    w = self._w3(self.effective_weight())
                    self._cache_packed = Fn.PreparedWeights(key, w, None, None, desc)
        return self._cache_packed

    def adopt_prepared(self, pw):
        """Take ``pw``, built elsewhere (weight_bank.WeightBank) under the current ``_params_key()``, as what
        ``prepared()`` returns until a parameter changes."""
        self._cache_packed = pw

    def holds_current(self, pw):
        """Is ``pw`` the instance this layer holds, and is it current?"""
        return self._cache_packed is pw and pw.key == self._params_key()

    def _packed(self, pack, cached):
        if self.has_spectral_norm and self.training:
            # every training-mode forward performs a power iteration: nothing to cache
            return pack(self.make_desc(1, self._probe_len()), self._w3(self.effective_weight()))
        return cached(self.prepared())

    def packed_weight(self):
        """Cached forward weight image (no-grad path)."""
        return self._packed(ops.pack_weight, lambda pw: pw.fwd)

    def packed_weight_bf16(self):
        """Cached bf16 weight image (bf16-operand inference), held by the same ``prepared()`` instance."""
        return self._packed(ops.pack_weight_bf16, lambda pw: pw.bf16())

    def packed_weight_split(self):
        """Cached split-operand weight images (fp32 inference on the bf16 MFMA), held by the same ``prepared()``."""
        return self._packed(ops.pack_weight_split, lambda pw: pw.split())

    def _split_route(self, desc, needs_grad=False):
        """Does this no-grad call (``desc``) of an fp32 module run on the split-operand kernel?"""
        cls = (desc.c_in, desc.c_out, desc.kernel, desc.batch * desc.t_out, needs_grad, self.split_exact,
               self.split_admit_all)
        return (split_admitted(*cls) or split_fewtap_admitted(*cls)) and ops.conv1d_split_supported(desc)

    def packed_weight_split_transposed(self):
        """Cached split-operand images of a k = 2s transposed layer, held by the same ``prepared()``."""
        return self._packed(ops.pack_weight_split_transposed, lambda pw: pw.split_transposed())

    def _upsample_split_route(self, desc, needs_grad=False):
        """Does this no-grad call (``desc``) of an fp32 transposed module run on the split-operand transposed kernel?"""
        return (self.transposed
                and upsample_split_admitted(desc.c_in, desc.c_out, desc.kernel, desc.stride, desc.batch * desc.t_out,
                                            needs_grad, self.split_exact, self.split_admit_all)
                and ops.convtr1d_split_supported(desc))

    def bf16_capable(self):
        """Does the bf16-operand kernel cover this layer's geometry (host logic, no device needed)?"""
        return not self.width_mode and ops.conv1d_bf16_supported(self.make_desc(1, self._probe_len()))

    @staticmethod
    def _w3(w):
        return w.reshape(w.shape[0], w.shape[1], -1).contiguous()

    def _probe_len(self):
        # any length with at least one output column (packing does not depend on it)
        return self.kernel_size * self.dilation + self.stride + max(0, -self.padding_right)

    def geom(self):
        return dict(kernel=self.kernel_size, stride=self.stride, dilation=self.dilation, padding=self.padding,
                    padding_right=self.padding_right, groups=self.groups, transposed=self.transposed,
                    output_padding=self.output_padding, width=1, pad_mode=self.pad_mode)

    def out_length(self, t_in):
        raise NotImplementedError

    def make_desc(self, batch, t_in, width=1, **fused):
        raise NotImplementedError

    def _needs_grad(self, *tensors):
        if not torch.is_grad_enabled():
            return False
        if any(p.requires_grad for p in self.parameters(recurse=False)):
            return True
        return any(t is not None and t.requires_grad for t in tensors)

    def _fold_batch(self, x, add1, add2, precomputed):
        """Few columns per item under a large weight (the 1024-channel tail of the scale discriminators at T = 9 .. 32,
        reference: models/hifigan.py:529-601): every item's workgroups stream the whole weight image for a handful of
        columns, and the launch takes the same ~80 us at T = 9, 17 and 32 (profiles/r05_tile_order_ab.txt).  A
        convolution along T treats the items exactly like the independent width columns of the period discriminators'
        (k, 1) layers, so such a layer runs as ONE item of width B over the activations transposed to (C, T, B):
        B x fewer passes over the weights, full column tiles, and the weight gradient's reduction chunks are full too.
        The transposing copies (2 x the activation bytes, a few MB) are the price."""
        if not self.fold_batch or self.width_mode or self.transposed or x.dim() != 3 or self.pad_mode != "zero":
            return False
        if add1 is not None or add2 is not None or precomputed is not None:
            return False
        b, t_out = x.shape[0], self.out_length(x.shape[-1])
        # (the layer's whole weight, groups included: restricting the rule to >= 4 MB PER GROUP -- i.e. to the k = 5 layer
        # -- because the grouped layers' forward measured 87 instead of 80 us stand-alone gave C3 -0.3 ms instead of
        # -1.1 ms and C5 -0.8 instead of -1.2 ms per captured step: their weight gradients gain more than that)
        w_bytes = 4 * self.out_channels * (self.in_channels // self.groups) * self.kernel_size
        return b >= 4 and 0 < t_out <= self.fold_max_cols and w_bytes >= self.fold_min_weight_bytes

    def forward(self, x, pre_act=None, pre_slope=0.0, post_act=None, post_slope=0.0, add1=None, add2=None,
                out_mul=1.0, out_div=1.0, precomputed=None):
        """Fused ``post((conv(pre(x)) + bias + add1 + add2) * out_mul / out_div)``.  ``precomputed`` (autograd path
        only): this layer's output as produced by a multi-layer kernel -- no launch, the node is recorded for backward."""
        if self._fold_batch(x, add1, add2, precomputed):
            b, c, t = x.shape
            xf = x.permute(1, 2, 0).contiguous().view(1, c, t, b)
            y = self._forward(xf, b, pre_act, pre_slope, post_act, post_slope, None, None, out_mul, out_div, None)
            return y.reshape(self.out_channels, -1, b).permute(2, 0, 1).contiguous()
        return self._forward(x, 0, pre_act, pre_slope, post_act, post_slope, add1, add2, out_mul, out_div, precomputed)

    def _forward(self, x, folded, pre_act, pre_slope, post_act, post_slope, add1, add2, out_mul, out_div, precomputed):
        """``folded``: 0, or the width of a batch-folded input (1, C, T, B) of a layer that is not in width mode."""
        fused = dict(pre_act=pre_act, pre_slope=pre_slope, post_act=post_act, post_slope=post_slope,
                     out_mul=out_mul, out_div=out_div)
        width_mode = self.width_mode or folded > 0
        if self.precision == "bf16" and self._needs_grad(x, add1, add2):
            raise bf16_no_backward_error(self, "HiFiGANGenerator")
        if self._needs_grad(x, add1, add2):
            geom = self.geom()
            if width_mode:
                geom["width"] = x.shape[-1]
            if self.pad_mode != "zero" and (self.padding > 0 or self.padding_right > 0):
                # the backward kernels implement zero padding: pad explicitly (HIP kernel with its own
                # backward); pad and the element-wise pre-activation commute
                x = Fn.pad1d(x, self.padding, self.padding_right, self.pad_mode)
                geom["padding"], geom["padding_right"], geom["pad_mode"] = 0, 0, "zero"
            if self.has_spectral_norm:
                # one power iteration per training forward: the weight is a fresh autograd node
                assert precomputed is None
                return Fn.FusedConvFn.apply(x, self.weight_tensor(), self.bias, add1, add2, geom, fused, None)
            if self.has_weight_norm:
                return Fn.FusedConvFn.apply(x, self.weight_v, self.bias, add1, add2, geom, fused, self.prepared(),
                                            self.weight_g, precomputed)
            return Fn.FusedConvFn.apply(x, self.weight, self.bias, add1, add2, geom, fused, self.prepared(), None,
                                        precomputed)
        assert precomputed is None, "precomputed outputs only make sense on the autograd path"
        with torch.no_grad():
            b = x.shape[0]
            if width_mode:
                h, width = x.shape[2], x.shape[3]
                desc = self.make_desc(b, h, width=width, **fused)
                y = ops.conv1d_forward(desc, x.reshape(b, x.shape[1], -1).contiguous(), self.packed_weight(),
                                       None if self.bias is None else self.bias.detach(),
                                       None if add1 is None else add1.reshape(b, self.out_channels, -1),
                                       None if add2 is None else add2.reshape(b, self.out_channels, -1))
                return y.reshape(b, self.out_channels, desc.t_out, width)
            if (self.pad_mode != "zero" and (self.padding > 0 or self.padding_right > 0) and not self.transposed
                    and x.numel() >= self.explicit_pad_min_elems):
                # Large inputs: pad explicitly (one streaming launch) and run the zero-padding LDS-DMA kernel -- what the
                # training path does anyway.  The register-staged kernel that maps reflected indices itself runs at
                # 33 - 41 TFLOP/s on MelGAN's residual stacks (96 channels, k = 3, B64 x T2048: 176 us) against 103 us
                # for the DMA kernel + 25 us for the pad (profiles/r04_k1_sweep.txt, r04_b_train_shapes_c4.txt).
                xp = Fn.pad1d(x, self.padding, self.padding_right, self.pad_mode)
                t_out = self.out_length(x.shape[-1])
                desc = ops.make_conv_desc(b, self.in_channels, self.out_channels, xp.shape[-1], t_out, self.kernel_size,
                                          self.stride, self.dilation, 0, self.groups, transposed=False, **fused)
                return ops.conv1d_forward(desc, xp, self.packed_weight(),
                                          None if self.bias is None else self.bias.detach(), add1, add2)
            desc = self.make_desc(b, x.shape[-1], **fused)
            if self.precision == "bf16" and ops.conv1d_bf16_supported(desc):
                return ops.conv1d_forward_bf16(desc, x.contiguous(), self.packed_weight_bf16(),
                                               None if self.bias is None else self.bias.detach(), add1, add2)
            if self.precision == "fp32" and self._split_route(desc):
                return ops.conv1d_forward_split(desc, x.contiguous(), self.packed_weight_split(),
                                                None if self.bias is None else self.bias.detach(), add1, add2)
            if self.precision == "fp32" and self._upsample_split_route(desc):
                return ops.conv1d_forward_split_transposed(desc, x.contiguous(), self.packed_weight_split_transposed(),
                                                           None if self.bias is None else self.bias.detach(), add1, add2)
            return ops.conv1d_forward(desc, x.contiguous(), self.packed_weight(),
                                      None if self.bias is None else self.bias.detach(), add1, add2)

    def extra_repr(self):
        norm = "weight_norm" if self.has_weight_norm else ("spectral_norm" if self.has_spectral_norm else "none")
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, "
                f"padding={self.padding}, dilation={self.dilation}, groups={self.groups}, norm={norm}")


# Admission table of the split-operand kernel: (c_in, c_out, kernel) -> fewest output columns per launch (batch x t_out)
# from which the class measured faster than the fp32 kernel by more than the spread of its repeated runs
# (profiles/split_infer.txt).  Classes not listed, and shorter launches, stay on the fp32 kernel.
# 6400 columns is the shortest launch measured on which each class wins (128 channels: one utterance of 100 frames,
# 1.30 - 1.36 x; 256 channels: one utterance of 800 frames, 1.04 - 1.07 x; at 800 columns the 256-channel classes lose
# 2 - 3 x).  16 x 800 frames: k = 7 1.46 x (128) / 1.56 x (256), k = 11 1.70 x / 1.73 x.
SPLIT_ADMITTED = {
    (128, 128, 7): 6400,
    (128, 128, 11): 6400,
    (256, 256, 7): 6400,
    (256, 256, 11): 6400,
}


def split_admitted(c_in, c_out, kernel, cols, needs_grad, enabled=True, admit_all=False):
    """The admission predicate of the split-operand kernel (pure host logic): never when a gradient is needed or the
    switch is off; else every class (``admit_all``) or the classes of ``SPLIT_ADMITTED`` from their column count on.
    What the kernel itself covers is ``ops.conv1d_split_supported``'s to say."""
    if needs_grad or not enabled:
        return False
    if admit_all:
        return True
    min_cols = SPLIT_ADMITTED.get((c_in, c_out, kernel))
    return min_cols is not None and cols >= min_cols


# Admission table of the split-operand kernel for the few-tap classes (k = 3), beside SPLIT_ADMITTED, which keeps the
# k >= 7 classes: (c_in, c_out, kernel) -> fewest output columns per launch (batch x t_out).  The rule is that of the
# tables around it: a class is listed when every run of the split kernel (in the form its launch plan chooses) at
# 16 x 800 frames was faster than every run of the fp32 kernel and the median gain was >= 1.25 x; its column count is the
# shortest measured launch (16 x 800, 1 x 800, 1 x 100 frames) on which it still won disjointly, and never under
# SPLIT_FEWTAP_MIN_COLS.  Classes not listed, and shorter launches, stay on the fp32 kernel.
# Both rows were measured on the staged window with the resident step, which is what the kernel's plan launches for them
# (profiles/split_window.txt B; DESIGN.md s9.1, "The prefetched window" and "The few-tap routing"): at 16 x 800 frames
# 128 -> 128 1.64 - 1.70 x, 256 -> 256 1.74 - 1.84 x, every run disjoint; at 6400 columns 1.90 x (128 channels, one utterance
# of 100 frames) and 1.26 x (256 channels, one utterance of 800 frames), disjoint; at 800 columns 256 -> 256 loses (0.79 x).
SPLIT_FEWTAP_MIN_COLS = 6400
SPLIT_FEWTAP_ADMITTED = {
    (128, 128, 3): 6400,
    (256, 256, 3): 6400,
}


def split_fewtap_admitted(c_in, c_out, kernel, cols, needs_grad, enabled=True, admit_all=False):
    """The admission predicate of the split-operand kernel for the few-tap classes (pure host logic), consulted after
    :func:`split_admitted` and honouring the same switches: never when a gradient is needed or the switch is off; else
    every class (``admit_all``) or the classes of ``SPLIT_FEWTAP_ADMITTED`` from their column count on."""
    if needs_grad or not enabled:
        return False
    if admit_all:
        return True
    min_cols = SPLIT_FEWTAP_ADMITTED.get((c_in, c_out, kernel))
    return min_cols is not None and cols >= max(min_cols, SPLIT_FEWTAP_MIN_COLS)


# Admission table of the split-operand transposed kernel (convtr1d_split_mfma_kernel; DESIGN.md s9.3,
# profiles/convtr_split.txt): (c_in, c_out, stride) of a ConvTranspose1d with kernel == 2 * stride -> fewest output
# columns per launch (batch x t_out).  The rule is that of the two tables around it: a class is listed when every run of
# the new kernel was faster than every run of the fp32 kernel and the median gain at 16 x 800 frames was >= 1.25 x; its
# column count is the shortest measured launch (16 x 800, 1 x 800, 1 x 100 frames) on which it still won disjointly,
# and never under UPSAMPLE_SPLIT_MIN_COLS, the shortest launch measured at all.  Classes not listed, and shorter
# launches, stay on the fp32 kernel.
# 16 x 800 frames: 1.77 x (512 -> 256), 2.28 x (256 -> 128), 1.93 x (128 -> 64), 1.94 x (64 -> 32), all disjoint.  One
# utterance of 800 frames: 512 -> 256 ties (0.99 x at 6400 columns) and loses at 100 frames (0.62 x), so it is admitted
# from the 16-utterance launch only; the other three still win disjointly at one utterance of 100 frames (1.17 x,
# 2.21 x, 1.73 x), the shortest launch measured.
UPSAMPLE_SPLIT_MIN_COLS = 800
UPSAMPLE_SPLIT_ADMITTED = {
    (512, 256, 8): 102400,
    (256, 128, 8): 6400,
    (128, 64, 2): 12800,
    (64, 32, 2): 25600,
}


def upsample_split_admitted(c_in, c_out, kernel, stride, cols, needs_grad, enabled=True, admit_all=False):
    """The admission predicate of the split-operand transposed kernel (pure host logic), the sibling of
    :func:`split_admitted`: never when a gradient is needed or the switch is off; else every k = 2s class
    (``admit_all``) or the classes of ``UPSAMPLE_SPLIT_ADMITTED`` from their column count on.  What the kernel itself
    covers is ``ops.convtr1d_split_supported``'s to say."""
    if needs_grad or not enabled or kernel != 2 * stride:
        return False
    if admit_all:
        return True
    min_cols = UPSAMPLE_SPLIT_ADMITTED.get((c_in, c_out, stride))
    return min_cols is not None and cols >= max(min_cols, UPSAMPLE_SPLIT_MIN_COLS)


# Admission table of the split-operand residual units (profiles/resunit_split.txt):
# (channels, kernel, has_conv2) -> (form, fewest columns per launch = batch x T).  form "unit": one launch of
# csrc/resunit_split.hip; form "pair": the two general split-operand launches of csrc/conv1d_split.hip that the unit
# kernel is defined by -- the same bits, and at 64 channels with k = 7 / 11 the faster of the two (1.00 / 1.40 ms
# against 1.15 / 1.71 ms per unit at 16 x 800 frames).  A class is listed when every run of its form was faster than
# every run of the incumbent (the fp32 unit; two fp32 convolutions at C = 64, k = 11) and the median gain at 16 x 800
# frames was >= 1.25 x; the column count is the shortest measured launch on which it still won disjointly, and never
# under RESUNIT_SPLIT_MIN_COLS.  C = 32, k = 3 gained 1.10 x when the table was filled and 1.27 - 1.28 x (disjoint) since
# the unit streams its weight fragments and requests its epilogue operands early (profiles/split_window.txt C); it wins
# disjointly down to 25600 columns and is listed from 51200, the shortest measured winning launch above the 25600 at
# which tests/test_hifigan_resunit_split_gpu.py pins the fp32 unit.  The single-convolution form was not measured and is
# not listed.  Classes not listed, and shorter launches, stay where they were.
RESUNIT_SPLIT_MIN_COLS = 20480
RESUNIT_SPLIT_ADMITTED = {
    (64, 3, True): ("unit", 20480),
    (64, 7, True): ("pair", 20480),
    (64, 11, True): ("pair", 20480),
    (32, 3, True): ("unit", 51200),
    (32, 7, True): ("unit", 25600),
    (32, 11, True): ("unit", 25600),
}


def resunit_split_admitted(channels, kernel, has_conv2, cols, needs_grad, enabled=True, admit_all=False):
    """The admission predicate of the split-operand residual units (pure host logic), the sibling of
    :func:`split_admitted`: None (never when a gradient is needed or the switch is off), else the form to run --
    ``"unit"`` for every unit under ``admit_all``, or what ``RESUNIT_SPLIT_ADMITTED`` lists for the class from its column
    count on.  What the kernels themselves cover is ``ops.resunit_split_supported`` / ``ops.conv1d_split_supported``'s
    to say."""
    if needs_grad or not enabled:
        return None
    if admit_all:
        return "unit"
    form, min_cols = RESUNIT_SPLIT_ADMITTED.get((channels, kernel, bool(has_conv2)), (None, 0))
    return form if form is not None and cols >= max(min_cols, RESUNIT_SPLIT_MIN_COLS) else None


# Admission table of the chained block of split-operand units (resblock_split_kernel of csrc/resunit_split.hip; DESIGN.md
# s9.2, "The chained block"; profiles/resblock_split.txt): (channels, kernel) -> (most units per launch, fewest columns
# per launch = batch x T).  A block of pair-form units all of which route to the one-launch split unit runs as ONE launch,
# the same bits.  The rule is that of the tables above: a class is listed when, at 16 x 800 frames, every run of the block
# was faster than every run of the unit launches it replaces, in each of three processes; its column count is the
# shortest measured launch (16 x 800, 1 x 800, 1 x 100 frames) from which it wins disjointly on.
# Both k = 3 classes pass in every process, with three units and with two (the block in front of a pending join): at
# 16 x 800 frames 1.22 - 1.23 x (C = 32, 1115 -> 910 us) and 1.06 - 1.07 x (C = 64, 1608 -> 1503 us), at 1 x 800 frames
# 1.30 - 1.35 x and 1.23 - 1.25 x.  Their floors are those 1 x 800 launches: the 1 x 100 launches lie under the floors of
# the units' own rows above, where the block has no split units to replace.  C = 32, k = 7 is disjointly slower with three
# units (0.90 x: 35 % more matrix work for the frame's discarded edge columns) and overlaps with two; C = 32, k = 11 loses
# (0.66 x); the 64-channel k = 7 / 11 units run as pairs, and their chain is refused by the kernel.  Not listed.
RESBLOCK_SPLIT_ADMITTED = {
    (32, 3): (3, 204800),
    (64, 3): (3, 102400),
}


def resblock_split_admitted(channels, kernel, n_units, cols, needs_grad, enabled=True):
    """The admission predicate of the chained block (pure host logic), beside :func:`resunit_split_admitted`: never
    when a gradient is needed or the split switch is off; else the classes of ``RESBLOCK_SPLIT_ADMITTED``, from two
    units up to their unit count and from their column count on.  ``split_admit_all`` does not reach it: that switch
    sends every unit to its one-launch kernel, which is what the tests that set it count.  Whether every unit of the
    block routes to the one-launch split unit is the caller's to check, what the kernel covers
    ``ops.resblock_split_supported``'s to say."""
    if needs_grad or not enabled or n_units < 2:
        return False
    max_units, min_cols = RESBLOCK_SPLIT_ADMITTED.get((channels, kernel), (0, 0))
    return n_units <= max_units and cols >= min_cols


def each_conv(module):
    """Every convolution module (:class:`_ConvNd`) of a module tree."""
    return (m for m in module.modules() if isinstance(m, _ConvNd))


def group_image(owner, slot, convs, pack, *extra):
    """The image that ``pack(w0, scale0, w1, scale1, ...)`` builds from the weights and weight-norm row scales of
    ``convs`` (a fused multi-layer kernel's operand), cached on ``owner`` under ``slot`` until a parameter of any of
    them changes; ``extra``: further key parts (what else the image depends on)."""
    key = extra + tuple(cv._params_key() for cv in convs)
    held = getattr(owner, slot, None)
    if held is None or held[0] != key:
        hs = [cv.prepared() for cv in convs]
        with torch.no_grad():
            held = (key, pack(*(t for h in hs for t in (h.w, h.scale))))
        setattr(owner, slot, held)
    return held[1]


def bf16_no_backward_error(module, model):
    """What a gradient-requiring call of a module in bf16 mode raises (``model``: the generator class whose
    ``inference(..., precision='bf16')`` is the intended entry)."""
    return RuntimeError(
        f"{module.__class__.__name__} is in bf16 inference precision, which has no backward pass: run it under "
        f"torch.no_grad() ({model}.inference(..., precision='bf16') does), or switch back with "
        "utils.set_inference_precision(model, 'fp32') before training")


class Conv1d(_ConvNd):
    """Drop-in for ``torch.nn.Conv1d`` (zero / reflect / replicate implicit padding)."""

    transposed = False

    def out_length(self, t_in):
        return ops.conv_out_length(t_in, self.kernel_size, self.stride, self.dilation, self.padding, self.padding_right)

    def make_desc(self, batch, t_in, width=1, **fused):
        return ops.make_conv_desc(batch, self.in_channels, self.out_channels, t_in, self.out_length(t_in),
                                  self.kernel_size, self.stride, self.dilation, self.padding, self.groups,
                                  transposed=False, width=width, pad_mode=self.pad_mode, **fused)


class Conv2d(Conv1d):
    """Drop-in for ``torch.nn.Conv2d`` restricted to ``(k, 1)`` kernels, ``(s, 1)`` strides and
    ``(p, 0)`` padding -- the only 2-D convolutions on the hot path (period discriminator,
    /root/reference/parallel_wavegan/models/hifigan.py:314-341).  Input (B, C, H, W); the
    weight keeps torch's (C_out, C_in, k, 1) shape."""

    width_mode = True

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True):
        def _first(v, name):
            if isinstance(v, (tuple, list)):
                if len(v) != 2 or (name == "kernel_size" and v[1] != 1) or (name == "stride" and v[1] != 1) or (
                        name == "padding" and v[1] != 0):
                    raise NotImplementedError(f"Conv2d: only (k,1) kernels / (s,1) strides / (p,0) padding, got {name}={v}")
                return v[0]
            if name == "stride":
                if v != 1:
                    raise NotImplementedError("Conv2d: an int stride > 1 would also stride the width axis")
                return 1
            raise NotImplementedError(f"Conv2d: {name} must be given as a (k, 1)-style tuple")

        super().__init__(in_channels, out_channels, _first(kernel_size, "kernel_size"), _first(stride, "stride"),
                         _first(padding, "padding"), bias=bias)

    def _weight_shape(self):
        return (self.out_channels, self.in_channels // self.groups, self.kernel_size, 1)


class ConvTranspose1d(_ConvNd):
    """Drop-in for ``torch.nn.ConvTranspose1d`` (polyphase; weight (C_in, C_out/groups, k))."""

    transposed = True

    def out_length(self, t_in):
        return ops.conv_transpose_out_length(t_in, self.kernel_size, self.stride, self.padding, self.output_padding)

    def make_desc(self, batch, t_in, width=1, **fused):
        return ops.make_conv_desc(batch, self.in_channels, self.out_channels, t_in, self.out_length(t_in),
                                  self.kernel_size, self.stride, 1, self.padding, self.groups, transposed=True,
                                  width=width, **fused)
