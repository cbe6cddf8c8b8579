"""Mel upsampling network of Parallel WaveGAN (drop-in names for parallel_wavegan.layers.upsample).

The reference materialises ``F.interpolate(nearest)`` and then runs a single-channel
``Conv2d(1, 1, (F, 2s+1))`` (+ an optional activation) per scale (layers/upsample.py:16-128); here each
scale is ONE HBM-bound HIP kernel (stretch + smoothing conv + activation fused, functional.StretchConvFn).  Parameter names
and shapes are kept (``up_layers.{1,3,..}.weight`` of shape (1, 1, 1, 2s+1), weight-normed by the
generator), so reference checkpoints load unchanged.
"""
import numpy as np
import torch

from .. import functional as Fn
from .. import ops
from .residual_block import Conv1d


class Stretch2d(torch.nn.Module):
    """Marker for the nearest-neighbour stretch (fused into the following Conv2d kernel)."""

    def __init__(self, x_scale, y_scale, mode="nearest"):
        super().__init__()
        if mode != "nearest" or y_scale != 1:
            raise NotImplementedError("only nearest stretching along time has a gfx950 kernel")
        self.x_scale, self.y_scale, self.mode = x_scale, y_scale, mode

    def forward(self, x):  # pragma: no cover
        raise RuntimeError("Stretch2d is fused into the smoothing convolution kernel")


class Conv2d(torch.nn.Module):
    """``Conv2d`` of the reference's upsampler (layers/upsample.py:47-59): weight initialised to 1 / prod(kernel_size),
    bias to 0.  On the hot path it is the single-channel (F, k) smoothing convolution that follows a ``Stretch2d`` and
    runs fused with it (``UpsampleNetwork.forward``); any other shape can be constructed and initialised (the
    reference's own unit test does) but has no stand-alone gfx950 kernel."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, bias=False, **kwargs):
        super().__init__()
        if kwargs:
            raise NotImplementedError(f"upsample Conv2d: unsupported arguments {sorted(kwargs)}")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        self.padding = padding
        self.weight = torch.nn.Parameter(torch.empty((out_channels, in_channels) + self.kernel_size))
        self.bias = torch.nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        self.weight.data.fill_(1.0 / np.prod(self.kernel_size))
        if self.bias is not None:
            torch.nn.init.constant_(self.bias, 0.0)

    @property
    def fusable(self):
        """(1 -> 1, no bias): the form ``UpsampleNetwork`` fuses with the preceding stretch."""
        return self.in_channels == 1 and self.out_channels == 1 and self.bias is None

    def forward(self, x):  # pragma: no cover
        raise NotImplementedError("upsample Conv2d runs fused with the preceding Stretch2d inside UpsampleNetwork; a "
                                  "stand-alone Conv2d has no gfx950 kernel")

    @property
    def has_weight_norm(self):
        return "weight_g" in self._parameters

    def apply_weight_norm(self):
        if not self.has_weight_norm:
            w = self._parameters.pop("weight")
            n0 = w.shape[0]
            self.weight_g = torch.nn.Parameter(w.detach().reshape(n0, -1).norm(dim=1).reshape(n0, 1, 1, 1).clone())
            self.weight_v = torch.nn.Parameter(w.detach().clone())
        return self

    def remove_weight_norm(self):
        if not self.has_weight_norm:
            raise ValueError("weight norm is not applied")
        g, v = self._parameters.pop("weight_g"), self._parameters.pop("weight_v")
        n0 = v.shape[0]
        self.weight = torch.nn.Parameter(v.detach() * (g.detach() / v.detach().reshape(n0, -1).norm(dim=1).reshape(n0, 1, 1, 1)))
        return self

    def weight_tensor(self):
        if self.has_weight_norm:
            return Fn.WeightNormFn.apply(self.weight_v, self.weight_g)
        return self.weight


_STAGE_ACTS = {"LeakyReLU": "leaky_relu", "ReLU": "relu", "Tanh": "tanh"}


class UpsampleNetwork(torch.nn.Module):
    """Stretch2d + (freq_axis_kernel_size, 2*scale+1) Conv2d [+ nonlinearity] per scale (layers/upsample.py:62-128);
    ``up_layers`` keeps the reference's indices (the activation modules carry no parameters)."""

    def __init__(self, upsample_scales, nonlinear_activation=None, nonlinear_activation_params={},
                 interpolate_mode="nearest", freq_axis_kernel_size=1, use_causal_conv=False):
        super().__init__()
        assert (freq_axis_kernel_size - 1) % 2 == 0, "Not support even number freq axis kernel size."
        self.use_causal_conv = use_causal_conv
        self.act, self.slope = None, 0.0
        if nonlinear_activation is not None:
            if nonlinear_activation not in _STAGE_ACTS:
                raise NotImplementedError(f"UpsampleNetwork: activation {nonlinear_activation!r} has no gfx950 epilogue "
                                          f"(supported: {sorted(_STAGE_ACTS)})")
            self.act = _STAGE_ACTS[nonlinear_activation]
            if self.act == "leaky_relu":
                self.slope = float(nonlinear_activation_params.get("negative_slope", 0.01))
                if not self.slope > 0.0:
                    raise NotImplementedError("UpsampleNetwork: LeakyReLU needs a positive slope (its gradient mask is "
                                              "taken from the stage output)")
        self.up_layers = torch.nn.ModuleList()
        self._stages = []
        freq_axis_padding = (freq_axis_kernel_size - 1) // 2
        for scale in upsample_scales:
            self._stages.append(len(self.up_layers))
            self.up_layers.append(Stretch2d(scale, 1, interpolate_mode))
            # causal: padding (., 2*scale) and the output trimmed to the stretched length
            # (layers/upsample.py:96-99,121-125) == left-only padding of 2*scale inside the kernel
            self.up_layers.append(Conv2d(1, 1, kernel_size=(freq_axis_kernel_size, scale * 2 + 1),
                                         padding=(freq_axis_padding, scale * 2 if use_causal_conv else scale), bias=False))
            if nonlinear_activation is not None:
                self.up_layers.append(getattr(torch.nn, nonlinear_activation)(**nonlinear_activation_params))

    def forward(self, c):
        """c: (B, C, T) -> (B, C, T * prod(upsample_scales))."""
        for i in self._stages:
            scale = self.up_layers[i].x_scale
            c = Fn.StretchConvFn.apply(c, self.up_layers[i + 1].weight_tensor(), scale,
                                       2 * scale if self.use_causal_conv else scale, self.act, self.slope)
        return c

    @torch.no_grad()
    def forward_ragged(self, c, frames, rate=1):
        """``forward`` over a ragged batch (inference): ``frames`` is the device int32 table of frames
        per item, ``rate`` the columns of ``c`` per frame; ``c`` must be exactly zero past every item's end, so that a
        stage reads there the zero padding it reads alone.  The same stage launches as ``forward``; ``ops.zero_tail``
        follows every stage whose output feeds another stage.  The last stage's output is left as it is past an item's
        end: its consumers read it point-wise."""
        if self.use_causal_conv:
            raise ValueError("UpsampleNetwork: a causal network has no ragged forward (it streams: stream_forward)")
        for k, i in enumerate(self._stages):
            scale = self.up_layers[i].x_scale
            c = Fn.StretchConvFn.apply(c, self.up_layers[i + 1].weight_tensor(), scale, scale, self.act, self.slope)
            rate *= scale
            if k + 1 < len(self._stages):
                ops.zero_tail(c, frames, rate)
        return c

    # ---- stateful streaming of the causal network (csrc/elementwise.hip, pwg_stretch_conv_stream)
    def stream_unsupported_reason(self):
        """None if every stage can be streamed, else the reason (host logic only)."""
        if not self.use_causal_conv:
            return "streaming needs use_causal_conv=True"
        return self._stage_geometry_reason()

    def _stage_geometry_reason(self):
        """What the stream kernel of a stage does not cover, causal or not."""
        for i in self._stages:
            if self.up_layers[i].mode != "nearest":
                return f"interpolate mode {self.up_layers[i].mode!r} (only 'nearest')"
            if self.up_layers[i + 1].kernel_size[0] != 1:
                return (f"freq_axis_kernel_size = {self.up_layers[i + 1].kernel_size[0]} (only 1: taps along the channel "
                        "axis are not built for streams)")
        return None

    def stream_layers(self, channels=80):
        """``(stage, rate)`` per upsampling stage in visiting order; ``rate``: the stage's input columns per input
        column of the network.  A stage keeps the last two raw input columns of every row (``channels`` rows per item:
        the network itself is agnostic of the mel width)."""
        reason = self.stream_unsupported_reason()
        if reason is not None:
            raise ValueError(f"{self.__class__.__name__}: {reason}")
        out, rate = [], 1
        for i in self._stages:
            out.append((StretchStageStream(self, i, channels), rate))
            rate *= self.up_layers[i].x_scale
        return out

    @torch.no_grad()
    def stream_forward(self, c, hist_in, hist_out):
        """The causal ``forward`` on the next chunk c (B, C, n) of a stream -> (B, C, n * prod(scales)); one launch per
        stage.  ``hist_in`` / ``hist_out``: one (B, C, 2) tensor per stage (``hist_in`` None: start of stream)."""
        stages = self.stream_layers()
        for k, (stage, _) in enumerate(stages):
            c = stage.stream_forward(c, None if hist_in is None else hist_in[k], hist_out[k])
        return c


    # ---- the NON-causal network streamed with a fixed look-ahead (pwg_stretch_conv_stream_delayed):
    # the stage y[u] = sum_j w[j] xs[u + j - s] is the causal stage (left padding 2 s) on a time axis shifted by s
    def lookahead_unsupported_reason(self):
        """None if every stage streams with a look-ahead, else the reason (host logic only)."""
        if self.use_causal_conv:
            return "the network is causal (use_causal_conv=True) and streams without look-ahead"
        return self._stage_geometry_reason()

    def lookahead_plan(self, channels, delay_in=0, rate=1):
        """One ``PWGLookaheadLaunch("stage", conv, rate, delay, 0, [(channels, 2)])`` per stage -> ``(launches, delay,
        rate)`` of the network's output: a stage of scale ``s`` takes an input delayed by ``D`` to ``D * s + s``."""
        from .causal_conv import PWGLookaheadLaunch

        reason = self.lookahead_unsupported_reason()
        if reason is not None:
            raise ValueError(f"{self.__class__.__name__}: {reason}")
        launches, delay = [], delay_in
        for i in self._stages:
            s = self.up_layers[i].x_scale
            delay, rate = delay * s + s, rate * s
            launches.append(PWGLookaheadLaunch("stage", self.up_layers[i + 1], rate, delay, 0, [(int(channels), 2)]))
        return launches, delay, rate

    @torch.no_grad()
    def lookahead_forward(self, c, walk, frames):
        """The non-causal ``forward`` on the next chunk of a look-ahead stream (``frames`` mel frames): one delayed
        launch per stage, state and valid window from ``walk`` (a :class:`layers.causal_conv.PWGLookaheadWalk`; a
        :class:`layers.causal_conv.PWGSlotWalk` hands out the slot table in the window's place: the slotted launch)."""
        from .causal_conv import pwg_stream_launch

        for i in self._stages:
            conv, scale = self.up_layers[i + 1], self.up_layers[i].x_scale
            _, ((hist_in, hist_out),), valid = walk.take("stage", conv, frames)
            c = pwg_stream_launch("stage", valid, c, hist_in, hist_out, conv.weight_tensor().detach(), scale,
                                  conv.kernel_size[0], self.act, self.slope)
        return c


class StretchStageStream:
    """One stage of a causal :class:`UpsampleNetwork` as a stateful stream layer (a view, no parameters of its own)."""

    def __init__(self, net, index, channels):
        self.net, self.index, self.channels = net, index, int(channels)
        self.scale = net.up_layers[index].x_scale

    def history_shape(self, batch):
        """Shape of one history buffer: the last two raw input columns (allocate two: ping-pong)."""
        return (batch, self.channels, 2)

    def history_columns_at_start(self):
        return 1  # zero-padded

    def stream_forward(self, c, hist_in, hist_out):
        conv = self.net.up_layers[self.index + 1]
        with torch.no_grad():
            return ops.stretch_conv_stream(c, hist_in, hist_out, conv.weight_tensor().detach(), self.scale,
                                           conv.kernel_size[0], self.net.act, self.net.slope)

    def __repr__(self):
        return f"StretchStageStream(scale={self.scale})"


class ConvInStream:
    """The causal ``conv_in`` of :class:`ConvInUpsampleNetwork` as a stateful stream layer: kernel
    ``aux_context_window + 1`` over the current frame and the ``aux_context_window`` frames before it.  The start of a
    stream replicates the first frame -- what ``inference()``'s replicate padding of the mel gives on the left (the
    right padding only feeds outputs the causal trim drops)."""

    def __init__(self, conv, context):
        self.conv, self.context = conv, int(context)

    def stream_desc(self, batch, n):
        cv = self.conv
        return ops.make_conv_desc(batch, cv.in_channels, cv.out_channels, n, n, cv.kernel_size, 1, 1, self.context, 1,
                                  transposed=False, pad_mode="replicate")

    def history_shape(self, batch):
        return (batch, self.conv.in_channels, self.context)

    def history_columns_at_start(self):
        return 1

    def stream_forward(self, c, hist_in, hist_out, precision="fp32"):
        from .causal_conv import _stream_forward

        return _stream_forward(self.conv, self.stream_desc(c.shape[0], c.shape[-1]), c, hist_in, hist_out, {}, precision)

    def __repr__(self):
        return f"ConvInStream({self.conv})"


class ConvInUpsampleNetwork(torch.nn.Module):
    """Context conv (k = 2*aux_context_window+1, no padding) + UpsampleNetwork (layers/upsample.py:131-194)."""

    def __init__(self, upsample_scales, nonlinear_activation=None, nonlinear_activation_params={},
                 interpolate_mode="nearest", freq_axis_kernel_size=1, aux_channels=80, aux_context_window=0,
                 use_causal_conv=False):
        super().__init__()
        self.aux_context_window = aux_context_window
        self.use_causal_conv = use_causal_conv and aux_context_window > 0
        # causal: kernel aux_context_window + 1 and the last aux_context_window outputs dropped
        # (layers/upsample.py:160-164,192-193): a negative right "padding" makes the kernel stop there
        kernel_size = aux_context_window + 1 if use_causal_conv else 2 * aux_context_window + 1
        self.conv_in = Conv1d(aux_channels, aux_channels, kernel_size=kernel_size, bias=False,
                              padding=(0, -aux_context_window) if self.use_causal_conv else 0)
        self.upsample = UpsampleNetwork(upsample_scales=upsample_scales, nonlinear_activation=nonlinear_activation,
                                        nonlinear_activation_params=nonlinear_activation_params,
                                        interpolate_mode=interpolate_mode, freq_axis_kernel_size=freq_axis_kernel_size,
                                        use_causal_conv=use_causal_conv)

    def forward(self, c):
        return self.upsample(self.conv_in(c))

    @torch.no_grad()
    def forward_ragged(self, c, frames):
        """``forward`` over a ragged batch (inference): ``c`` (B, C, T_pad + 2 * aux_context_window)
        holds item ``b``'s context-padded frames at the columns ``[0, frames[b] + 2 * aux_context_window)`` and anything
        past them.  ``conv_in`` runs as in ``forward``; its output is item ``b``'s at the columns ``< frames[b]`` and
        ``ops.zero_tail`` zeroes the rest (write-only: NaN included), then the stages run ragged."""
        if self.use_causal_conv:
            raise ValueError("ConvInUpsampleNetwork: a causal network has no ragged forward (it streams: stream_forward)")
        return self.upsample.forward_ragged(ops.zero_tail(self.conv_in(c), frames, 1), frames)

    # ---- stateful streaming of the causal network
    def stream_layers(self):
        """``(layer, rate)`` of the stateful layers in visiting order: ``conv_in`` (history: the last
        ``aux_context_window`` frames; absent without a context window), then the upsampling stages."""
        stages = self.upsample.stream_layers(self.conv_in.out_channels)  # ValueError for a non-causal network
        if self.aux_context_window > 0:
            return [(ConvInStream(self.conv_in, self.aux_context_window), 1)] + stages
        return stages

    @torch.no_grad()
    def stream_forward(self, c, hist_in, hist_out, precision="fp32"):
        """The causal ``forward`` on the next frames c (B, C, n) of a stream (frame t of the stream is column
        ``t + aux_context_window`` of the whole-utterance input) -> (B, C, n * prod(scales)).  ``hist_in`` / ``hist_out``:
        one tensor per layer of :meth:`stream_layers` (``hist_in`` None: start of stream, ``conv_in`` replicates the first
        frame).  ``precision``: of ``conv_in``'s launch; the stretch stages are fp32 in either."""
        k = 0
        if self.aux_context_window > 0:
            layer = ConvInStream(self.conv_in, self.aux_context_window)
            c = layer.stream_forward(c, None if hist_in is None else hist_in[0], hist_out[0], precision)
            k = 1
        else:
            from .causal_conv import stream_pointwise

            c = stream_pointwise(self.conv_in, c, precision)
        return self.upsample.stream_forward(c, None if hist_in is None else hist_in[k:], hist_out[k:])

    # ---- the NON-causal network streamed with a fixed look-ahead
    def _lookahead_desc(self, batch, n):
        """``conv_in`` (kernel 2 w + 1, no padding, on the replicate-padded mel) in causal form: left padding 2 w."""
        cv = self.conv_in
        return ops.make_conv_desc(batch, cv.in_channels, cv.out_channels, n, n, cv.kernel_size, 1, 1, cv.kernel_size - 1, 1,
                                  transposed=False, pad_mode="zero")

    def lookahead_plan(self):
        """``conv_in`` (history ``2 w`` frames, output ``w`` frames late), then the stages -> ``(launches, delay, rate)``."""
        from .causal_conv import PWGLookaheadLaunch

        if self.use_causal_conv:
            raise ValueError(f"{self.__class__.__name__}: the network is causal (use_causal_conv=True) and streams "
                             "without look-ahead")
        cv, w = self.conv_in, self.aux_context_window
        first = PWGLookaheadLaunch("conv_in", cv, 1, w, 0, [(cv.in_channels, 2 * w)] if w > 0 else [])
        launches, delay, rate = self.upsample.lookahead_plan(cv.out_channels, w, 1)
        return [first] + launches, delay, rate

    @torch.no_grad()
    def lookahead_forward(self, c, walk):
        """The non-causal ``forward`` on the next frames c (B, C, n) of a look-ahead stream -> (B, C, n * prod(scales)),
        late by the plan's delay.  The start of a stream replicates the first frame into ``conv_in``'s history (what
        ``inference()``'s replicate padding gives on the left); the end is the caller's: it feeds copies of the last
        frame.  ``conv_in`` runs in the walk's precision; the stretch stages are fp32 in either.  A slotted walk
        (:class:`layers.causal_conv.PWGSlotWalk`): the start of a stream is an item's, so the seeding kernel replicates
        the first frame of the fresh running items into the input history, and ``conv_in`` runs over the second table."""
        from .causal_conv import SlotPosition, lookahead_launch

        cv, w, n = self.conv_in, self.aux_context_window, c.shape[-1]
        _, pairs, valid = walk.take("conv_in", cv, n)
        hist_in, hist_out = pairs[0] if pairs else (None, None)
        if pairs and isinstance(valid, SlotPosition):
            ops.slot_seed_history(c, hist_in, valid.seed)
        elif pairs and hist_in is None:
            hist_in = c[:, :, :1].expand(-1, -1, 2 * w).contiguous()
        c = lookahead_launch(cv, self._lookahead_desc(c.shape[0], n), c, (hist_in, hist_out), valid, walk.precision)
        return self.upsample.lookahead_forward(c, walk, n)
