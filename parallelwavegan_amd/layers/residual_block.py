"""Residual blocks (drop-in names for parallel_wavegan.layers.residual_block)."""
import math

import torch

from .. import _lib
from .. import functional as Fn
from .. import ops
from .activation import FusedActivation
from .conv import Conv1d as _Conv1d
from .conv import bf16_no_backward_error, group_image, resblock_split_admitted, resunit_split_admitted


from .causal_conv import (CausalConv1d, LookaheadLaunch, lookahead_delay,  # noqa: E402  (depends on .conv only)
                          pwg_stream_launch)
from .dropout import Dropout as _Dropout  # noqa: E402


class Conv1d(_Conv1d):
    """Conv1d with the reference's customised initialisation (kaiming normal for ReLU, zero bias;
    layers/residual_block.py:19-30)."""

    def reset_parameters(self):
        w = self.raw_weight
        fan_in = int(w[0].numel())
        with torch.no_grad():
            w.normal_(0.0, math.sqrt(2.0 / fan_in))  # kaiming_normal_(nonlinearity="relu"), fan_in mode
            if self.bias is not None:
                self.bias.zero_()


class Conv1d1x1(Conv1d):
    def __init__(self, in_channels, out_channels, bias):
        super().__init__(in_channels, out_channels, kernel_size=1, padding=0, dilation=1, bias=bias)


class WaveNetResidualBlock(torch.nn.Module):
    """Gated residual block of the PWG generator (layers/residual_block.py:43-140): dilated conv ->
    + aux 1x1 -> tanh * sigmoid -> skip 1x1 and out 1x1 (+ residual) * sqrt(0.5).  Five launches (+1 for the dropout mask when ``dropout > 0`` in training):
    aux conv, dilated conv (+aux fused as addend), gate, skip conv (+running skip sum fused), out conv
    (+residual and the sqrt(0.5) scale fused)."""

    def __init__(self, kernel_size=3, residual_channels=64, gate_channels=128, skip_channels=64, aux_channels=80,
                 dropout=0.0, dilation=1, bias=True, use_causal_conv=False):
        super().__init__()
        self.dropout = dropout
        self._drop = _Dropout(dropout)  # parameter-free: no state-dict entries
        self.use_causal_conv = use_causal_conv
        if use_causal_conv:
            # the reference pads (k-1)*d on both sides and drops the future part of the output
            # (layers/residual_block.py:74-76,118-119): identical to left-only padding
            padding = ((kernel_size - 1) * dilation, 0)
        else:
            assert (kernel_size - 1) % 2 == 0, "Not support even number kernel size."
            padding = (kernel_size - 1) // 2 * dilation
        self.conv = Conv1d(residual_channels, gate_channels, kernel_size, padding=padding, dilation=dilation,
                           bias=bias)
        self.conv1x1_aux = Conv1d1x1(aux_channels, gate_channels, bias=False) if aux_channels > 0 else None
        gate_out_channels = gate_channels // 2
        self.conv1x1_out = Conv1d1x1(gate_out_channels, residual_channels, bias=bias)
        self.conv1x1_skip = Conv1d1x1(gate_out_channels, skip_channels, bias=bias)
        for cv in self.fused_convs():
            if cv is not None:
                cv.bank_images = False  # weight_bank.WeightBank: row scales only; the layer's own fused image is used

    fuse_layer = True  # one launch per layer where csrc/wavenet.hip covers the geometry (PWG.v1: 64 / 128 / 64 / 80)

    # ---- the one-launch layer (csrc/wavenet.hip)
    def fused_convs(self):
        return (self.conv, self.conv1x1_aux, self.conv1x1_skip, self.conv1x1_out)

    def fused_params(self):
        """Parameters in the order WaveNetLayerFn returns their gradients."""
        ps = []
        for cv in self.fused_convs():
            ps.append(cv.raw_weight)
            if cv.has_weight_norm:
                ps.append(cv.weight_g)
            if cv.bias is not None:
                ps.append(cv.bias)
        return ps

    def fused_desc(self, batch, t, skip_scale=1.0):
        return ops.make_wavenet_desc(batch, t, self.conv.dilation, self.conv.in_channels, self.conv.out_channels,
                                     self.conv1x1_skip.out_channels,
                                     0 if self.conv1x1_aux is None else self.conv1x1_aux.in_channels,
                                     self.conv.kernel_size, self.use_causal_conv, math.sqrt(0.5), skip_scale)

    def fused_image(self):
        """MFMA A-operand image of the layer's four weights for the current parameter values."""
        return group_image(self, "_fused_img", self.fused_convs(),
                           lambda *ws: ops.wavenet_pack_weights(self.fused_desc(1, 64), *ws))

    def fused_image_bwd(self, skip_scale=1.0):
        """Backward-pass image (gate / dilated / aux data gradients) for the current parameter values."""
        return group_image(self, "_fused_bwd_img", self.fused_convs(),
                           lambda *ws: ops.wavenet_pack_weights_bwd(self.fused_desc(1, 64, skip_scale), *ws),
                           float(skip_scale))

    def _fusable(self, x, c):
        if not self.fuse_layer or c is None or self.conv1x1_aux is None or x.dim() != 3 or not x.is_cuda:
            return False
        if self.use_causal_conv or (self.dropout > 0.0 and self.training):
            return False
        if any(cv.has_spectral_norm or cv.pad_mode != "zero" for cv in self.fused_convs()):
            return False
        if self.conv1x1_out.out_channels != self.conv.in_channels:
            return False
        return ops.wavenet_layer_supported(self.fused_desc(x.shape[0], x.shape[2]))

    # ---- bf16-operand inference (csrc/wavenet_bf16.hip): the whole layer in one launch, any dilation
    def _bf16_geometry_reason(self, batch=1, t=1):
        """None if the fused bf16 layer covers this block at (batch, t), else the reason it does not."""
        if self.conv1x1_aux is None:
            return "the block has no aux (conditioning) convolution"
        if self.use_causal_conv:
            return "causal layers are not built"
        if any(cv.has_spectral_norm or cv.pad_mode != "zero" for cv in self.fused_convs()):
            return "spectral norm or non-zero padding"
        if self.conv1x1_out.out_channels != self.conv.in_channels:
            return "out channels differ from the residual channels"
        if not ops.wavenet_bf16_supported(self.fused_desc(batch, t)):
            return _lib.lib().pwg_last_error().decode(errors="replace")
        return None

    def bf16_covered_convs(self):
        """Convolutions that the fused bf16 layer runs in bf16 although the stand-alone bf16 kernel may not cover them
        (the dilation-512 dilated convolution): all four when the layer geometry is covered, else none.  Asked by
        ``utils.set_inference_precision``; host logic only."""
        return tuple(self.fused_convs()) if self._bf16_geometry_reason() is None else ()

    def fused_image_bf16(self):
        """bf16 MFMA image of the layer's four weights, cached like ``fused_image``."""
        return group_image(self, "_fused_bf16_img", self.fused_convs(),
                           lambda *ws: ops.wavenet_bf16_pack_weights(self.fused_desc(1, 64), *ws))

    def _forward_bf16(self, x, c, skips, skip_scale, chain_aux, inplace_skips):
        """Some convolution of the block is in bf16 mode: the fused bf16 launch when all four are and it covers the
        call, else the per-convolution path -- where every bf16 convolution must run in bf16 on its own kernel."""
        convs = [cv for cv in self.fused_convs() if cv is not None]
        if any(cv._needs_grad(x, c, skips) for cv in convs):
            raise bf16_no_backward_error(self, "ParallelWaveGANGenerator")
        all_bf16 = all(cv.precision == "bf16" for cv in convs)
        reason = None
        if not all_bf16:
            reason = "its convolutions are in mixed precision"
        elif c is None:
            reason = "no aux input"
        elif x.dim() != 3 or not x.is_cuda:
            reason = "the input is not a (B, C, T) device tensor"
        elif self.dropout > 0.0 and self.training:
            reason = "dropout in training mode"
        else:
            reason = self._bf16_geometry_reason(x.shape[0], x.shape[2])
        if reason is None:
            with torch.no_grad():
                b_d, b_s, b_o = (None if cv.bias is None else cv.bias.detach()
                                 for cv in (self.conv, self.conv1x1_skip, self.conv1x1_out))
                x_out, s_out, _, _ = ops.wavenet_bf16_layer_forward(
                    self.fused_desc(x.shape[0], x.shape[2], skip_scale), x.contiguous(), c.contiguous(), skips,
                    self.fused_image_bf16(), b_d, b_s, b_o, skips_out=skips if inplace_skips else None)
            return (x_out, s_out, c) if chain_aux else (x_out, s_out)
        # per-convolution path: a bf16 convolution the stand-alone kernel cannot take is an error, not an fp32 run
        t = x.shape[-1]
        for name, cv in (("conv", self.conv), ("conv1x1_aux", self.conv1x1_aux), ("conv1x1_skip", self.conv1x1_skip),
                         ("conv1x1_out", self.conv1x1_out)):
            if cv is not None and cv.precision == "bf16" and not ops.conv1d_bf16_supported(cv.make_desc(x.shape[0], t)):
                why = _lib.lib().pwg_last_error().decode(errors="replace")
                raise RuntimeError(f"{self.__class__.__name__}: {name} is in bf16 inference precision, but the fused bf16 "
                                   f"layer cannot run this call ({reason}) and the bf16 convolution kernel does not cover "
                                   f"it ({why})")
        return None

    # ---- stateful streaming of the causal block (csrc/wavenet_stream.hip): one launch per chunk
    def history_shape(self, batch):
        """Shape of one history buffer: the last ``(k - 1) * d`` raw input columns (allocate two: ping-pong)."""
        return (batch, self.conv.in_channels, (self.conv.kernel_size - 1) * self.conv.dilation)

    def history_columns_at_start(self):
        return 1  # (zero-padded: the first push needs nothing but itself)

    def stream_desc(self, batch, n, skip_scale=1.0):
        """Descriptor of one push of ``n`` columns through the streaming layer kernel."""
        return self.fused_desc(batch, n, skip_scale)

    def stream_unsupported_reason(self, batch=1, n=1, precision="fp32"):
        """None if the streaming layer kernel of ``precision`` covers this block at (batch, n), else the reason it does
        not (host logic only).  A non-causal block is not a geometry question: ``stream_forward`` raises ValueError for
        it."""
        if self.conv1x1_aux is None:
            return "the block has no aux (conditioning) convolution"
        if any(cv.has_spectral_norm or cv.pad_mode != "zero" for cv in self.fused_convs()):
            return "spectral norm or non-zero padding"
        if self.conv1x1_out.out_channels != self.conv.in_channels:
            return "out channels differ from the residual channels"
        supported = ops.wavenet_stream_bf16_supported if precision == "bf16" else ops.wavenet_stream_supported
        if not supported(self.stream_desc(batch, n)):
            return _lib.lib().pwg_last_error().decode(errors="replace")
        return None

    def stream_image(self):
        """The layer's fp32 weight image for the streaming kernel: the image of ``fused_image`` -- its row order (tap 0,
        1, 2, aux) does not depend on causality -- packed through a non-causal descriptor of the same channels, because
        the packer's geometry check admits only the layers its own forward covers."""
        def pack(*ws):
            d = self.fused_desc(1, 64)
            d.causal = 0
            return ops.wavenet_pack_weights(d, *ws)

        return group_image(self, "_stream_img", self.fused_convs(), pack)

    def stream_image_bf16(self):
        """The layer's bf16 weight image for the bf16 streaming kernel (csrc/wavenet_stream_bf16.hip): the image of
        ``fused_image_bf16`` -- its K order (tap 0, 1, 2, aux) does not depend on causality -- packed through a
        non-causal descriptor of the same channels, as ``stream_image`` is; cached under a key of its own."""
        def pack(*ws):
            d = self.fused_desc(1, 64)
            d.causal = 0
            return ops.wavenet_bf16_pack_weights(d, *ws)

        return group_image(self, "_stream_bf16_img", self.fused_convs(), pack)

    def _stream_precision(self, precision):
        """The precision of a stream call, by the rule of ``layers.causal_conv._stream_forward``: a bf16 call neither
        reads nor writes the modules' own ``precision`` attributes (whole-utterance mode); an fp32 call refuses a block
        in bf16 mode."""
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"stream precision must be 'fp32' or 'bf16', got {precision!r}")
        if precision == "fp32" and any(cv is not None and cv.precision != "fp32" for cv in self.fused_convs()):
            raise RuntimeError("WaveNetResidualBlock is in bf16 inference precision: the fp32 streaming layer kernel does "
                               "not read that mode (utils.set_inference_precision(model, 'fp32'), or pass "
                               "precision='bf16' to stream with bf16 operands)")
        return precision == "bf16"

    def stream_forward(self, x, c, hist_in, hist_out, skips=None, skip_scale=1.0, inplace_skips=False, precision="fp32"):
        """The causal block on the next ``x.shape[-1]`` columns of a stream whose previous columns are ``hist_in`` (None:
        start of stream, zero left context) -> (x_out, skips + s); also writes ``hist_out`` (a buffer distinct from
        ``hist_in``).  One launch.  ``inplace_skips``: the new running sum is written into ``skips``.
        ``precision="bf16"``: the same launch with bf16 operands (csrc/wavenet_stream_bf16.hip) on the block's bf16
        image; the history stays raw fp32, so the state of a stream does not depend on its precision."""
        if not self.use_causal_conv:
            raise ValueError("WaveNetResidualBlock: streaming needs use_causal_conv=True")
        bf16 = self._stream_precision(precision)
        reason = self.stream_unsupported_reason(x.shape[0], x.shape[-1], precision) if x.dim() == 3 else "x is not (B, C, n)"
        if reason is None and self.dropout > 0.0 and self.training:
            reason = "dropout in training mode"
        if reason is not None:
            raise RuntimeError("the streaming layer kernel does not cover this block: " + reason)
        with torch.no_grad():
            b_d, b_s, b_o = (None if cv.bias is None else cv.bias.detach()
                             for cv in (self.conv, self.conv1x1_skip, self.conv1x1_out))
            forward = ops.wavenet_stream_forward_bf16 if bf16 else ops.wavenet_stream_forward
            return forward(self.stream_desc(x.shape[0], x.shape[-1], skip_scale), x.contiguous(), c.contiguous(), skips,
                           hist_in, hist_out, self.stream_image_bf16() if bf16 else self.stream_image(), b_d, b_s, b_o,
                           skips_out=skips if (inplace_skips and skips is not None) else None)

    # ---- the NON-causal block streamed with a fixed look-ahead (csrc/wavenet_stream.hip, the delayed form; DESIGN.md
    # s11.6): the causal launch on a time axis shifted by the dilation
    def lookahead_unsupported_reason(self, batch=1, n=1, c_delay=0, precision="fp32"):
        """None if the delayed form of the streaming layer kernel of ``precision`` covers this non-causal block at
        (batch, n) with the conditioning read ``c_delay`` columns late, else the reason it does not (host logic only).
        A causal block is not a geometry question: ``lookahead_forward`` raises ValueError for it."""
        if self.conv1x1_aux is None:
            return "the block has no aux (conditioning) convolution"
        if any(cv.has_spectral_norm or cv.pad_mode != "zero" for cv in self.fused_convs()):
            return "spectral norm or non-zero padding"
        if self.conv1x1_out.out_channels != self.conv.in_channels:
            return "out channels differ from the residual channels"
        supported = ops.wavenet_stream_delayed_bf16_supported if precision == "bf16" else \
            ops.wavenet_stream_delayed_supported
        if not supported(self.fused_desc(batch, n), c_delay):
            return _lib.lib().pwg_last_error().decode(errors="replace")
        return None

    def lookahead_forward(self, x, c, c_line, c_delay, hist, skips=None, skip_line=(None, None), valid=None,
                          skip_scale=1.0, precision="fp32"):
        """The non-causal block on the next ``x.shape[-1]`` columns of a look-ahead stream -> (x_out, skips + s), both
        ``dilation`` columns later than ``x``.  ``hist = (hist_in, hist_out)``: the last ``2 * dilation`` columns of the
        block's input (``hist_in`` None: start of stream); the conditioning is read ``c_delay`` columns late from
        ``concat(c_line, c)``; the running skip sum goes through ``skip_line = (line_in, line_out)`` of ``dilation``
        columns; columns outside ``valid = (lo, hi)`` are stored as zeros -- a ``causal_conv.SlotPosition`` in its place
        (a pool's walk): the slotted launch, every item at its own position.  One launch.  ``precision="bf16"``: the same
        launch with bf16 operands (csrc/wavenet_stream_bf16.hip); history and lines stay raw fp32."""
        if self.use_causal_conv:
            raise ValueError("WaveNetResidualBlock: a causal block streams without look-ahead (stream_forward, "
                             "utils.PWGStream)")
        bf16 = self._stream_precision(precision)
        reason = self.lookahead_unsupported_reason(x.shape[0], x.shape[-1], c_delay, precision) if x.dim() == 3 \
            else "x is not (B, C, n)"
        if reason is None and self.dropout > 0.0 and self.training:
            reason = "dropout in training mode"
        if reason is not None:
            raise RuntimeError("the delayed streaming layer kernel does not cover this block: " + reason)
        with torch.no_grad():
            b_d, b_s, b_o = (None if cv.bias is None else cv.bias.detach()
                             for cv in (self.conv, self.conv1x1_skip, self.conv1x1_out))
            return pwg_stream_launch("layer", valid, self.fused_desc(x.shape[0], x.shape[-1], skip_scale), x.contiguous(),
                                     c.contiguous(), c_line, c_delay, skips, skip_line, hist[0], hist[1],
                                     self.stream_image_bf16() if bf16 else self.stream_image(), b_d, b_s, b_o,
                                     precision="bf16" if bf16 else "fp32")

    # ---- utterances of different lengths in one batch (the ragged forms of csrc/wavenet.hip and csrc/wavenet_bf16.hip;
    # DESIGN.md s9.6): one launch, no per-convolution path
    def ragged_unsupported_reason(self, batch=1, t=64, rate=4):
        """None if the ragged layer kernel of the block's precision covers it at (batch, t) and ``rate`` columns per
        frame, else the reason it does not (host logic only)."""
        if self.conv1x1_aux is None:
            return "the block has no aux (conditioning) convolution"
        if not self.fuse_layer:
            return "fuse_layer is off (the ragged block is the one-launch layer)"
        if self.use_causal_conv:
            return "causal layers are not built"
        if any(cv.has_spectral_norm or cv.pad_mode != "zero" for cv in self.fused_convs()):
            return "spectral norm or non-zero padding"
        if self.conv1x1_out.out_channels != self.conv.in_channels:
            return "out channels differ from the residual channels"
        if len({cv.precision for cv in self.fused_convs()}) != 1:
            return "its convolutions are in mixed precision"
        if self.dropout > 0.0 and self.training:
            return "dropout in training mode"
        if not ops.wavenet_layer_ragged_supported(self.fused_desc(batch, t), rate):
            return _lib.lib().pwg_last_error().decode(errors="replace")
        return None

    @torch.no_grad()
    def forward_ragged(self, x, c, frames, rate, skips=None, skip_scale=1.0, inplace_skips=False):
        """``forward`` over a ragged batch (inference) -> (x_out, skips + s): ``frames`` is the device int32 table of
        frames per item, ``rate`` the columns of ``x`` per frame.  ONE ragged launch, fp32 or bf16 by the convolutions'
        precision as ``forward`` chooses; ``x``, ``c`` and ``skips`` may hold anything past an item's end, and the outputs
        are not written there.  ValueError with the reason for a block the kernel does not cover: there is no
        per-convolution path."""
        reason = self.ragged_unsupported_reason(x.shape[0], x.shape[-1], rate) if x.dim() == 3 else "x is not (B, C, T)"
        if reason is not None:
            raise ValueError("WaveNetResidualBlock.forward_ragged: the ragged layer kernel does not cover this block: "
                             + reason)
        bf16 = self.conv.precision == "bf16"
        b_d, b_s, b_o = (None if cv.bias is None else cv.bias.detach()
                         for cv in (self.conv, self.conv1x1_skip, self.conv1x1_out))
        return ops.wavenet_layer_forward_ragged(
            self.fused_desc(x.shape[0], x.shape[-1], skip_scale), x.contiguous(), c.contiguous(), skips, frames, rate,
            self.fused_image_bf16() if bf16 else self.fused_image(), b_d, b_s, b_o,
            skips_out=skips if (inplace_skips and skips is not None) else None, bf16=bf16)

    def forward(self, x, c, skips=None, skip_scale=1.0, chain_aux=False, inplace_skips=False):
        """Returns (x_out, skips + s) -- the running skip sum is an addend of the skip conv's epilogue
        (``skip_scale`` is the final ``sqrt(1/layers)`` of the generator, applied by the last block).
        ``inplace_skips``: the no-grad fused path may write the new running sum into ``skips`` itself.
        ``chain_aux``: also return the aux features for the NEXT layer (the same values; on the one-launch autograd
        path an alias whose gradient is chained through the layers' data-gradient epilogues)."""
        if any(cv is not None and cv.precision == "bf16" for cv in self.fused_convs()):
            out = self._forward_bf16(x, c, skips, skip_scale, chain_aux, inplace_skips)
            if out is not None:
                return out
        elif self._fusable(x, c):
            needs_grad = torch.is_grad_enabled() and (x.requires_grad or c.requires_grad
                                                      or (skips is not None and skips.requires_grad)
                                                      or any(p.requires_grad for p in self.fused_params()))
            if needs_grad:
                x_out, s_out, c_next = Fn.WaveNetLayerFn.apply(x, c, skips, self, skip_scale, *self.fused_params())
                return (x_out, s_out, c_next) if chain_aux else (x_out, s_out)
            with torch.no_grad():
                convs = self.fused_convs()
                b_d, b_s, b_o = (None if cv.bias is None else cv.bias.detach() for cv in (convs[0], convs[2], convs[3]))
                x_out, s_out, _, _ = ops.wavenet_layer_forward(self.fused_desc(x.shape[0], x.shape[2], skip_scale),
                                                               x.contiguous(), c.contiguous(), skips, self.fused_image(),
                                                               b_d, b_s, b_o,
                                                               # the running skip sum is updated in place only when the caller
                                                               # owns that buffer and says so (the generator's own loop)
                                                               skips_out=skips if inplace_skips else None)
                return (x_out, s_out, c) if chain_aux else (x_out, s_out)
        aux = self.conv1x1_aux(c) if (c is not None and self.conv1x1_aux is not None) else None
        # F.dropout on the dilated conv's input only; the residual path keeps x (residual_block.py:114-116)
        z = self.conv(self._drop(x), add1=aux)
        g = Fn.GateFn.apply(z)
        s = self.conv1x1_skip(g, add1=skips, out_mul=skip_scale)
        x = self.conv1x1_out(g, add1=x, out_mul=math.sqrt(0.5))
        return (x, s, c) if chain_aux else (x, s)


class HiFiGANResidualBlock(torch.nn.Module):
    """MRF residual block: ``x = x + conv_{k,1}(act(conv_{k,d}(act(x))))`` per dilation.

    Same constructor / state-dict keys as the reference's
    ``HiFiGANResidualBlock`` (/root/reference/parallel_wavegan/layers/residual_block.py:143-258);
    the forward issues two fused HIP launches per dilation (activation, bias and
    the residual add live inside the convolution kernels).
    """

    def __init__(self, kernel_size=3, channels=512, dilations=(1, 3, 5), bias=True, use_additional_convs=True,
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1},
                 use_causal_conv=False):
        super().__init__()
        assert kernel_size % 2 == 1, "Kernel size must be odd number."
        self.use_additional_convs = use_additional_convs
        self.use_causal_conv = use_causal_conv
        self.kernel_size = kernel_size
        self.dilations = tuple(dilations)
        self.convs1 = torch.nn.ModuleList()
        if use_additional_convs:
            self.convs2 = torch.nn.ModuleList()
        def conv(dilation):
            # causal: left-only padding inside CausalConv1d (layers/residual_block.py:196-241 of the reference)
            if use_causal_conv:
                return CausalConv1d(channels, channels, kernel_size, dilation=dilation, bias=bias)
            return Conv1d(channels, channels, kernel_size, 1, dilation=dilation, bias=bias,
                          padding=(kernel_size - 1) // 2 * dilation)

        for d in self.dilations:
            self.convs1.append(torch.nn.Sequential(
                FusedActivation(nonlinear_activation, **nonlinear_activation_params), conv(d)))
            if use_additional_convs:
                self.convs2.append(torch.nn.Sequential(
                    FusedActivation(nonlinear_activation, **nonlinear_activation_params), conv(1)))

    # inference: one launch per unit where csrc/resunit.hip (fp32 MFMA) or csrc/resunit_split.hip (bf16 MFMA, split
    # operands; admitted classes only) covers the geometry (C = 32 / 64)
    fuse_units = True

    def _unit_route(self, idx, x, accum, out_div):
        """How ``forward`` runs unit ``idx`` on ``x``: None (separate convolutions: training, where the intermediate is
        needed by the backward pass; causal / wide layers, which have no resident-tile kernel) or ``(form, desc, d1, d2)``
        -- ``form``: ``"unit"`` (csrc/resunit_split.hip), ``"pair"`` (two split launches, descriptors ``d1`` / ``d2``) or
        None (the fp32 unit, csrc/resunit.hip); ``desc``: the unit's descriptor.  One decision for ``forward`` and
        ``forward_ragged``."""
        act1, conv1 = self.convs1[idx][0], self.convs1[idx][1]
        if (not self.fuse_units or self.use_causal_conv or act1.kind != "leaky_relu" or x.dim() != 3
                or not x.is_cuda or conv1._needs_grad(x, None if callable(accum) else accum)):
            return None
        slope2, conv2 = act1.slope, None
        if self.use_additional_convs:
            act2, conv2 = self.convs2[idx][0], self.convs2[idx][1]
            if act2.kind != "leaky_relu" or conv2._needs_grad(x) or conv2.has_spectral_norm:
                return None
            slope2 = act2.slope
        if conv1.has_spectral_norm or conv1.pad_mode != "zero":
            return None
        if conv1.precision != "fp32" or (conv2 is not None and conv2.precision != "fp32"):
            return None  # bf16-operand inference: the unit's convolutions run one by one on csrc/conv1d_bf16.hip
        desc = ops.make_resunit_desc(x.shape[0], x.shape[1], x.shape[2], self.kernel_size, conv1.dilation,
                                     conv2 is not None, act1.slope, slope2, out_div)
        # the split-operand forms: the same unit on the bf16 MFMA where the class is admitted, as one
        # launch of csrc/resunit_split.hip or as the pair of general split launches it is defined by (same bits).  A
        # gradient is never needed here: checked above
        convs = (conv1,) if conv2 is None else (conv1, conv2)
        form = resunit_split_admitted(x.shape[1], self.kernel_size, conv2 is not None, x.shape[0] * x.shape[2], False,
                                      all(cv.split_exact for cv in convs), all(cv.split_admit_all for cv in convs))
        if form == "unit" and not ops.resunit_split_supported(desc):
            form = None
        d1 = d2 = None
        if form == "pair":
            b, t = x.shape[0], x.shape[2]
            d1 = conv1.make_desc(b, t, pre_act="leaky_relu", pre_slope=act1.slope, post_act="leaky_relu",
                                 post_slope=slope2)
            d2 = conv2.make_desc(b, t, out_div=out_div)
            if not (ops.conv1d_split_supported(d1) and ops.conv1d_split_supported(d2)):
                form = None
        if form is None and not ops.resunit_profitable(desc):
            return None
        return form, desc, d1, d2

    def _unit_one_launch(self, idx, x, accum, out_div):
        """``(x + convs2[idx](convs1[idx](x)) [+ accum]) [/ out_div]`` as ONE kernel launch (two for the ``"pair"``
        form), or None when :meth:`_unit_route` sends the unit to its separate convolutions."""
        route = self._unit_route(idx, x, accum, out_div)
        if route is None:
            return None
        form, desc, d1, d2 = route
        conv1 = self.convs1[idx][1]
        conv2 = self.convs2[idx][1] if self.use_additional_convs else None
        if callable(accum):
            accum = accum()  # (resolved as late as possible: it may wait for another stream)
        with torch.no_grad():
            x = x.contiguous()
            accum = None if accum is None else accum.contiguous()
            b1 = None if conv1.bias is None else conv1.bias.detach()
            b2 = None if (conv2 is None or conv2.bias is None) else conv2.bias.detach()
            if form == "unit":
                return ops.resunit_forward_split(desc, x, conv1.packed_weight_split(), b1,
                                                 None if conv2 is None else conv2.packed_weight_split(), b2, accum)
            if form == "pair":
                h = ops.conv1d_forward_split(d1, x, conv1.packed_weight_split(), b1)
                return ops.conv1d_forward_split(d2, h, conv2.packed_weight_split(), b2, x, accum)
            return ops.resunit_forward(
                desc, x, conv1.prepared().res(), None if conv1.bias is None else conv1.bias.detach(),
                None if conv2 is None else conv2.prepared().res(),
                None if (conv2 is None or conv2.bias is None) else conv2.bias.detach(),
                None if accum is None else accum.contiguous())

    # inference: a block whose units all run as one-launch split units runs as ONE launch where its class is admitted
    # (resblock_split_kernel of csrc/resunit_split.hip; layers/conv.py, RESBLOCK_SPLIT_ADMITTED): the same bits
    fuse_block = True

    def _block_one_launch(self, x, m, accum, out_div):
        """The first ``m`` units on ``x`` as ONE launch of the chained block: ``(m, result)``, or ``(0, x)`` where
        the block stays on its unit loop -- the switch is off, the class is not admitted, or some unit of the ``m``
        would not run as a one-launch split unit.  ``m == len(self.convs1)``: the whole block, with ``accum`` and
        ``out_div`` in the last unit's epilogue; fewer: units ``0 .. m - 1`` as the loop runs them, no addend."""
        n = len(self.convs1)
        if (not self.fuse_block or not self.fuse_units or self.use_causal_conv or not self.use_additional_convs
                or m < 2 or x.dim() != 3):
            return 0, x  # (a causal block has no resident-tile kernel, and its convolutions no split switch)
        whole = m == n
        convs = [cv[1] for cv in self.convs1[:m]] + [cv[1] for cv in self.convs2[:m]]
        # (before any unit is asked: the predicate is a table look-up, a unit's route builds descriptors)
        if not resblock_split_admitted(x.shape[1], self.kernel_size, m, x.shape[0] * x.shape[2], False,
                                       all(cv.split_exact for cv in convs)):
            return 0, x
        routes = [self._unit_route(idx, x, accum if whole and idx == n - 1 else None,
                                   out_div if whole and idx == n - 1 else 1.0) for idx in range(m)]
        if any(r is None or r[0] != "unit" for r in routes):
            return 0, x
        desc = routes[-1][1]  # batch, channels, t, kernel and the last unit's out_div: what the block reads of it
        dilations = [r[1].dilation for r in routes]
        if not ops.resblock_split_supported(desc, dilations):
            return 0, x
        with torch.no_grad():
            bias = lambda cv: None if cv.bias is None else cv.bias.detach()
            c1, c2 = convs[:m], convs[m:]
            return m, ops.resblock_forward_split(
                desc, x.contiguous(), dilations, [r[1].slope1 for r in routes], [r[1].slope2 for r in routes],
                [cv.packed_weight_split() for cv in c1], [bias(cv) for cv in c1],
                [cv.packed_weight_split() for cv in c2], [bias(cv) for cv in c2],
                None if not whole or accum is None else accum.contiguous())

    def forward(self, x, accum=None, out_div=1.0, accum_join=None):
        """``accum_join``: optional callable evaluated right before the block's last kernel, returning ``accum``
        (streams.run_branches_chained: the previous MRF branch is only waited for there).
        Returns ``(block(x) + accum) / out_div``; accum/out_div let the caller fold the
        MRF sum ``cs += block(c); c = cs / num_blocks`` (models/hifigan.py:186-190 in the
        reference) into this block's last kernel."""
        n = len(self.convs1)
        if accum_join is not None and not getattr(accum_join, "pending", True):
            accum, accum_join = accum_join(), None  # a join that waits for nothing: resolved here, the block may fuse
        # the chained block: all units in one launch, or, in front of a pending join, all but the last
        # one -- the previous MRF branch is still waited for only in front of the block's last kernel
        first, fused = self._block_one_launch(x, n if accum_join is None else n - 1, accum, out_div)
        if first == n:
            return fused
        x = fused

        def acc():
            """the addend of the last kernel, resolved right before that kernel is launched"""
            nonlocal accum, accum_join
            if accum_join is not None:
                accum, accum_join = accum_join(), None
            return accum

        for idx in range(first, n):
            last = idx == n - 1
            act1, conv1 = self.convs1[idx][0], self.convs1[idx][1]
            # (a pending join is passed on as a callable and resolved right before the launch)
            y = self._unit_one_launch(idx, x, (acc if accum_join is not None else accum) if last else None,
                                      out_div if last else 1.0)
            if y is not None:
                x = y
                continue
            if self.use_additional_convs:
                act2, conv2 = self.convs2[idx][0], self.convs2[idx][1]
                if not self.use_causal_conv and not (conv1._needs_grad(x) or conv2._needs_grad(x, accum)):
                    # inference: the intermediate has one consumer, so its activation is applied ONCE by the
                    # producer's epilogue instead of on every operand read of the consumer (k reads per
                    # element, 2 VALU ops each inside the MFMA loop); same fp32 values either way
                    xt = conv1(x, pre_act=act1.kind, pre_slope=act1.slope, post_act=act2.kind, post_slope=act2.slope)
                    x = conv2(xt, add1=x, add2=acc() if last else None, out_div=out_div if last else 1.0)
                    continue
                xt = conv1(x, pre_act=act1.kind, pre_slope=act1.slope)
                x = conv2(xt, pre_act=act2.kind, pre_slope=act2.slope, add1=x,
                          add2=acc() if last else None, out_div=out_div if last else 1.0)
            else:
                x = conv1(x, pre_act=act1.kind, pre_slope=act1.slope, add1=x,
                          add2=acc() if last else None, out_div=out_div if last else 1.0)
        return x

    @torch.no_grad()
    def forward_ragged(self, x, frames, rate, accum=None, out_div=1.0):
        """``forward`` over a ragged batch (inference): ``frames`` is the device int32 table of frames per
        item, ``rate`` the columns of ``x`` per frame; ``x`` and ``accum`` are zero past their items' ends and so is the
        result.  The same modules, order and fused epilogues as ``forward``, serial.  A unit ``forward`` sends to
        csrc/resunit_split.hip runs that kernel's ragged form where it is covered (``rate % 4 == 0``) and else the chain of
        split launches it is defined by; the ``"pair"`` form runs its two split launches; the fp32 unit and every unit
        ``forward`` does not fuse run as their separate convolutions, each with the route it takes on its own.  Every
        launch but the ragged unit's is followed by ``ops.zero_tail``."""
        if self.use_causal_conv:
            raise ValueError("HiFiGANResidualBlock: a causal block has no ragged forward (it streams: stream_forward)")
        n = len(self.convs1)
        for idx in range(n):
            last = idx == n - 1
            act1, conv1 = self.convs1[idx][0], self.convs1[idx][1]
            conv2 = self.convs2[idx][1] if self.use_additional_convs else None
            add2, div = (accum, out_div) if last else (None, 1.0)
            route = self._unit_route(idx, x, add2, div)
            form, desc, d1, d2 = route if route is not None else (None,) * 4
            b1 = None if conv1.bias is None else conv1.bias.detach()
            b2 = None if (conv2 is None or conv2.bias is None) else conv2.bias.detach()
            if form == "unit" and not ops.resunit_split_ragged_supported(desc, rate):
                # the chain of general split launches the unit is defined by (the same bits)
                slope2 = self.convs2[idx][0].slope if conv2 is not None else act1.slope
                if conv2 is not None:
                    d1 = conv1.make_desc(x.shape[0], x.shape[2], pre_act="leaky_relu", pre_slope=act1.slope,
                                         post_act="leaky_relu", post_slope=slope2)
                    d2 = conv2.make_desc(x.shape[0], x.shape[2], out_div=div)
                else:
                    d1 = conv1.make_desc(x.shape[0], x.shape[2], pre_act="leaky_relu", pre_slope=act1.slope, out_div=div)
                form = "pair" if all(ops.conv1d_split_supported(dd) for dd in (d1, d2) if dd is not None) else None
            if form == "unit":
                x = ops.resunit_forward_split_ragged(desc, x.contiguous(), frames, rate, conv1.packed_weight_split(),
                                                     b1, None if conv2 is None else conv2.packed_weight_split(), b2,
                                                     None if add2 is None else add2.contiguous())
            elif form == "pair":  # the split launches ``forward`` runs, the intermediate zeroed between them
                x, add2 = x.contiguous(), None if add2 is None else add2.contiguous()
                if conv2 is None:
                    y = ops.conv1d_forward_split(d1, x, conv1.packed_weight_split(), b1, x, add2)
                else:
                    h = ops.zero_tail(ops.conv1d_forward_split(d1, x, conv1.packed_weight_split(), b1), frames, rate)
                    y = ops.conv1d_forward_split(d2, h, conv2.packed_weight_split(), b2, x, add2)
                x = ops.zero_tail(y, frames, rate)
            elif conv2 is not None:
                act2 = self.convs2[idx][0]
                xt = conv1(x, pre_act=act1.kind, pre_slope=act1.slope, post_act=act2.kind, post_slope=act2.slope)
                ops.zero_tail(xt, frames, rate)
                x = ops.zero_tail(conv2(xt, add1=x, add2=add2, out_div=div), frames, rate)
            else:
                x = ops.zero_tail(conv1(x, pre_act=act1.kind, pre_slope=act1.slope, add1=x, add2=add2, out_div=div),
                                  frames, rate)
        return x

    def stream_layers(self):
        """The causal convolutions in the order :meth:`walk_forward` visits them."""
        out = []
        for idx in range(len(self.convs1)):
            out.append(self.convs1[idx][1])
            if self.use_additional_convs:
                out.append(self.convs2[idx][1])
        return out

    def lookahead_plan(self, delay_in, rate, delay_accum=None):
        """Delay plan of the NON-causal block streamed with a look-ahead (layers/causal_conv.py; host only) ->
        ``(launches, delay_out)``: one :class:`LookaheadLaunch` per convolution in the order :meth:`walk_forward`
        runs them.  ``delay_in``: delay of the block's input; ``rate``: its columns per mel frame; ``delay_accum``: delay
        of the MRF running sum added by the block's last launch (None: no sum yet).  The residual input of a unit is
        older than the unit's output by the paddings of its convolutions; the running sum by the difference of the block
        delays, which must not be negative."""
        if self.use_causal_conv:
            raise ValueError("HiFiGANResidualBlock: a causal block streams without look-ahead (stream_forward)")
        launches, dx, n = [], delay_in, len(self.convs1)
        for idx in range(n):
            d_out = d1 = lookahead_delay(self.convs1[idx][1], dx)
            if self.use_additional_convs:
                d_out = lookahead_delay(self.convs2[idx][1], d1)
                launches.append(LookaheadLaunch(self.convs1[idx][1], rate, d1, 0, 0))
            delay2 = 0
            if idx == n - 1 and delay_accum is not None:
                delay2 = d_out - delay_accum
                if delay2 < 0:
                    raise ValueError(
                        f"the MRF blocks of a stage must have non-decreasing delays to stream with a look-ahead: a block "
                        f"of kernel {self.kernel_size}, dilations {self.dilations} (delay {d_out - delay_in} columns) "
                        f"follows one with delay {delay_accum - delay_in} (order resblock_kernel_sizes ascending)")
            last_conv = self.convs2[idx][1] if self.use_additional_convs else self.convs1[idx][1]
            launches.append(LookaheadLaunch(last_conv, rate, d_out, d_out - dx, delay2))
            dx = d_out
        return launches, dx

    def walk_forward(self, x, walk, accum=None, out_div=1.0):
        """The block on the next chunk of a stream: the modules, order and fused epilogues of ``forward``, every
        convolution one launch through ``walk`` -- a :class:`layers.causal_conv.CausalWalk` over :meth:`stream_layers`
        (the causal block), or a ``LookaheadWalk`` / ``SlotWalk`` over the launches of :meth:`lookahead_plan` (the
        NON-causal block in causal form), which delays the addends."""
        n = len(self.convs1)
        for idx in range(n):
            last = idx == n - 1
            act1, conv1 = self.convs1[idx][0], self.convs1[idx][1]
            if self.use_additional_convs:
                act2, conv2 = self.convs2[idx][0], self.convs2[idx][1]
                xt = walk.run(conv1, x, pre_act=act1.kind, pre_slope=act1.slope)
                x = walk.run(conv2, xt, add1=x, add2=accum if last else None, pre_act=act2.kind, pre_slope=act2.slope,
                             out_div=out_div if last else 1.0)
            else:
                x = walk.run(conv1, x, add1=x, add2=accum if last else None, pre_act=act1.kind, pre_slope=act1.slope,
                             out_div=out_div if last else 1.0)
        return x
