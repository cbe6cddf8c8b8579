"""Parallel WaveGAN modules on the gfx950 kernel library (drop-in for
``parallel_wavegan.models.parallel_wavegan``; reference: models/parallel_wavegan.py)."""
import logging
import math

import numpy as np
import torch

from .. import functional as Fn
from .. import ops
from ..layers import upsample
from ..layers.activation import FusedActivation
from ..layers.conv import Conv1d as _AnyConv1d
from ..layers.residual_block import Conv1d, Conv1d1x1
from ..layers.residual_block import WaveNetResidualBlock as ResidualBlock
from ..layers.upsample import Conv2d as UpsampleConv2d


def _norm_modules(module):
    # every Conv1d / Conv2d of the tree, as the reference's ``isinstance(m, torch.nn.Conv1d) or ... Conv2d``
    # (models/parallel_wavegan.py:187-195): includes the convolutions of a MelGAN upsampler, not its
    # transposed convolutions
    for m in module.modules():
        if isinstance(m, (_AnyConv1d, UpsampleConv2d)):
            yield m


class _WeightNormMixin:
    def remove_weight_norm(self):
        for m in _norm_modules(self):
            if m.has_weight_norm:
                m.remove_weight_norm()
                logging.debug(f"Weight norm is removed from {m}.")

    def apply_weight_norm(self):
        for m in _norm_modules(self):
            m.apply_weight_norm()
            logging.debug(f"Weight norm is applied to {m}.")


class ParallelWaveGANGenerator(torch.nn.Module, _WeightNormMixin):
    """Non-autoregressive WaveNet generator (reference: models/parallel_wavegan.py:21-261)."""

    def __init__(self, in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=64,
                 gate_channels=128, skip_channels=64, aux_channels=80, aux_context_window=2, dropout=0.0, bias=True,
                 use_weight_norm=True, use_causal_conv=False, upsample_conditional_features=True,
                 upsample_net="ConvInUpsampleNetwork", upsample_params={"upsample_scales": [4, 4, 4, 4]}):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.aux_channels, self.aux_context_window = aux_channels, aux_context_window
        self.layers, self.stacks, self.kernel_size = layers, stacks, kernel_size
        assert layers % stacks == 0
        layers_per_stack = layers // stacks
        self.first_conv = Conv1d1x1(in_channels, residual_channels, bias=True)
        if upsample_conditional_features:
            upsample_params = dict(upsample_params)
            upsample_params.update({"use_causal_conv": use_causal_conv})
            if upsample_net == "MelGANGenerator":
                # a MelGAN generator as the mel upsampler (models/parallel_wavegan.py:90-98 of the reference):
                # its out_channels must equal aux_channels; weight norm is applied once, by this model
                assert aux_context_window == 0
                from .melgan import MelGANGenerator

                upsample_params.update({"use_weight_norm": False, "use_final_nonlinear_activation": False})
                self.upsample_net = MelGANGenerator(**upsample_params)
            else:
                if upsample_net == "ConvInUpsampleNetwork":
                    upsample_params.update({"aux_channels": aux_channels, "aux_context_window": aux_context_window})
                self.upsample_net = getattr(upsample, upsample_net)(**upsample_params)
            self.upsample_factor = int(np.prod(upsample_params["upsample_scales"]))
        else:
            self.upsample_net = None
            self.upsample_factor = 1
        self.conv_layers = torch.nn.ModuleList()
        for layer in range(layers):
            self.conv_layers.append(ResidualBlock(
                kernel_size=kernel_size, residual_channels=residual_channels, gate_channels=gate_channels,
                skip_channels=skip_channels, aux_channels=aux_channels, dilation=2 ** (layer % layers_per_stack),
                dropout=dropout, bias=bias, use_causal_conv=use_causal_conv))
        self.last_conv_layers = torch.nn.ModuleList([
            FusedActivation("ReLU"),
            Conv1d1x1(skip_channels, skip_channels, bias=True),
            FusedActivation("ReLU"),
            Conv1d1x1(skip_channels, out_channels, bias=True),
        ])
        if use_weight_norm:
            self.apply_weight_norm()

    def forward(self, z, c):
        """z: noise (B, 1, T), c: mel (B, C, T' + 2*aux_context_window) -> (B, out_channels, T)."""
        if c is not None and self.upsample_net is not None:
            c = self.upsample_net(c)
            assert c.size(-1) == z.size(-1)
        x = self.first_conv(z)
        skips = None
        n = len(self.conv_layers)
        for i, f in enumerate(self.conv_layers):
            # `skips += h` and the final `skips *= sqrt(1/n)` ride on the skip conv's epilogue
            # (c is handed from layer to layer so that its gradient is summed along that chain, see WaveNetLayerFn)
            x, skips, c = f(x, c, skips=skips, skip_scale=math.sqrt(1.0 / n) if i == n - 1 else 1.0, chain_aux=True,
                            inplace_skips=True)
        x = self.last_conv_layers[1](skips, pre_act="relu")
        return self.last_conv_layers[3](x, pre_act="relu")

    # ---- utterances of different lengths in one batch (utils.PWGRaggedSynthesizer)
    def ragged_unsupported_reason(self, precision="fp32"):
        """None if ``forward_ragged`` runs this generator in ``precision`` (``"fp32"`` / ``"bf16"``: both layer kernels
        have a ragged form of the same geometry), else the reason (host logic only)."""
        if precision not in ("fp32", "bf16"):
            return f"precision must be 'fp32' or 'bf16', got {precision!r}"
        if any(f.use_causal_conv for f in self.conv_layers):
            return "the model is causal (use_causal_conv=True): it streams (utils.PWGStream)"
        if self.upsample_net is None:
            return "upsample_conditional_features=False: an item's length is its mel frames through the upsampler"
        if not isinstance(self.upsample_net, (upsample.UpsampleNetwork, upsample.ConvInUpsampleNetwork)):
            return (f"upsample_net={self.upsample_net.__class__.__name__!r} has no ragged forward here (only "
                    "UpsampleNetwork and ConvInUpsampleNetwork)")
        if self.in_channels != 1 or self.out_channels != 1:
            return (f"in_channels = {self.in_channels}, out_channels = {self.out_channels}: an item takes one noise row "
                    "and returns one waveform")
        for i, f in enumerate(self.conv_layers):
            reason = f.ragged_unsupported_reason(1, 64, self.upsample_factor)
            if reason is not None:
                return f"conv_layers[{i}]: {reason}"
        return None

    @torch.no_grad()
    def forward_ragged(self, z, c, frames):
        """``forward`` over utterances of different lengths in one batch (the batched form of the loop of
        bin/decode.py:214-243 of the reference).  With ``w = aux_context_window`` and ``up =
        upsample_factor``: noise ``z`` (B, 1, T_pad * up), mel ``c`` (B, C, T_pad + 2 w), ``frames`` a device int32 tensor
        (B,) with ``0 <= frames[b] <= T_pad`` -> (B, 1, T_pad * up).  Item ``b`` of ``c`` holds its frames at the columns
        ``[w, w + frames[b])`` with its first and last frame replicated ``w`` columns outward (the caller pads, as
        ``forward``'s does); anything may sit past column ``frames[b] + 2 w`` of ``c`` and past ``frames[b] * up`` of
        ``z``, NaN included.  The columns ``< frames[b] * up`` of the output are what ``forward`` gives for the item
        alone; the rest is unspecified.  Neither ``z`` nor ``c`` is written.

        ``conv_in`` and the stretch stages run as in ``forward`` with ``ops.zero_tail`` behind every launch that feeds
        another stage; every gated layer is ONE ragged launch that reads nothing at or past an item's end and writes
        nothing there, so no zero-tail pass runs between layers; ``first_conv`` and the two last 1 x 1 convolutions are
        point-wise.  Nothing on the host reads the table: one captured graph per (B, T_pad) serves every set of
        lengths.  ValueError with the reason for a generator, shapes or a table this does not take."""
        name = "ParallelWaveGANGenerator.forward_ragged"
        reason = self.ragged_unsupported_reason()
        if reason is not None:
            raise ValueError(f"{name}: {reason}")
        w, up = self.aux_context_window, self.upsample_factor
        if not isinstance(self.upsample_net, upsample.ConvInUpsampleNetwork):
            w = 0  # (no context convolution: a mel column is a frame)
        if c.dim() != 3 or c.shape[1] != self.aux_channels or c.shape[2] <= 2 * w:
            raise ValueError(f"{name}: expected (B, {self.aux_channels}, T_pad + {2 * w}) features, got {tuple(c.shape)}")
        t_pad = c.shape[2] - 2 * w
        if tuple(z.shape) != (c.shape[0], 1, t_pad * up):
            raise ValueError(f"{name}: expected ({c.shape[0]}, 1, {t_pad * up}) noise for {tuple(c.shape)} features, got "
                             f"{tuple(z.shape)}")
        ops._require_device(z, c)
        if (not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.int32
                or tuple(frames.shape) != (c.shape[0],) or not frames.is_contiguous()):
            raise ValueError(f"{name}: the frames table must be a contiguous device int32 tensor of shape "
                             f"({c.shape[0]},), got {getattr(frames, 'dtype', type(frames).__name__)} "
                             f"{tuple(getattr(frames, 'shape', ()))} on {getattr(frames, 'device', 'the host')}")
        if isinstance(self.upsample_net, upsample.ConvInUpsampleNetwork):
            c = self.upsample_net.forward_ragged(c, frames)
        else:
            c = self.upsample_net.forward_ragged(ops.zero_tail(c.clone(), frames, 1), frames)
        x = self.first_conv(z)
        skips = None
        n = len(self.conv_layers)
        for i, f in enumerate(self.conv_layers):
            x, skips = f.forward_ragged(x, c, frames, up, skips=skips,
                                        skip_scale=math.sqrt(1.0 / n) if i == n - 1 else 1.0, inplace_skips=True)
        x = self.last_conv_layers[1](skips, pre_act="relu")
        return self.last_conv_layers[3](x, pre_act="relu")

    # ---- stateful streaming of the causal generator (utils.PWGStream)
    def stream_unsupported_reason(self, batch=1, precision="fp32"):
        """None if the causal generator can be streamed layer by layer in ``precision``, else the reason (host logic
        only)."""
        if not all(f.use_causal_conv for f in self.conv_layers):
            return "streaming needs use_causal_conv=True"
        if self.upsample_net is None:
            return "upsample_conditional_features=False: the stream maps mel frames to samples through the upsampler"
        if not isinstance(self.upsample_net, (upsample.UpsampleNetwork, upsample.ConvInUpsampleNetwork)):
            return (f"upsample_net={self.upsample_net.__class__.__name__!r} is not built for streams (only UpsampleNetwork "
                    "and ConvInUpsampleNetwork)")
        net = self.upsample_net.upsample if isinstance(self.upsample_net, upsample.ConvInUpsampleNetwork) \
            else self.upsample_net
        reason = net.stream_unsupported_reason()
        if reason is not None:
            return "the mel upsampler: " + reason
        for f in self.conv_layers:
            reason = f.stream_unsupported_reason(batch, 8, precision)
            if reason is not None:
                return f"{f.__class__.__name__}: {reason}"
        return None

    def pointwise_convs(self):
        """The 1 x 1 convolutions the causal stream runs through the conv stream kernel without history, in the order it
        visits them (``conv_in`` is one of them when there is no context window)."""
        convs = [self.first_conv, self.last_conv_layers[1], self.last_conv_layers[3]]
        if isinstance(self.upsample_net, upsample.ConvInUpsampleNetwork) and self.upsample_net.aux_context_window == 0:
            convs.insert(0, self.upsample_net.conv_in)
        return convs

    def stream_layers(self):
        """``(layer, rate)`` of every stateful layer in the order :meth:`stream_forward` visits them: the upsampler's
        (``conv_in``, then one per stage), then the residual blocks; ``rate``: the layer's input columns per mel frame."""
        reason = self.stream_unsupported_reason()
        if reason is not None:
            raise ValueError(f"{self.__class__.__name__}: {reason}")
        if isinstance(self.upsample_net, upsample.ConvInUpsampleNetwork):
            out = self.upsample_net.stream_layers()
        else:
            out = self.upsample_net.stream_layers(self.aux_channels)
        return out + [(f, self.upsample_factor) for f in self.conv_layers]

    @torch.no_grad()
    def stream_forward(self, z, c, hist_in, hist_out, precision="fp32"):
        """The causal ``forward`` on the next chunk of a stream: noise z (B, 1, n * upsample_factor) and mel frames
        c (B, C, n) -- frame t of the stream is column ``t + aux_context_window`` of the whole-utterance input -- ->
        (B, out_channels, n * upsample_factor).  The same modules in the same order: the upsampler's stream launches, the
        1 x 1 convolutions through the streaming kernel (its sum order does not depend on n), one launch per residual
        block; the running skip sum is updated in place and the last block applies sqrt(1 / layers).  ``hist_in`` /
        ``hist_out``: one history tensor per layer of :meth:`stream_layers` (``hist_in`` None: start of stream); see
        :class:`utils.PWGStream`.  ``precision="bf16"``: ``conv_in``, the 1 x 1 convolutions and the residual blocks run
        with bf16 operands; the stretch stages and every history stay fp32."""
        from ..layers.causal_conv import CausalWalk, stream_pointwise

        layers = self.stream_layers()
        walk = CausalWalk(layers, hist_in, hist_out, precision)  # (the lists' lengths; this model runs its layers itself)
        hist = [walk.take(layer) for layer, _ in layers]
        n, n_up = len(self.conv_layers), len(hist) - len(self.conv_layers)
        # (the upsampler takes its layers' pairs as two lists; a None entry is its start of stream too)
        up_in, up_out = [h_in for h_in, _ in hist[:n_up]], [h_out for _, h_out in hist[:n_up]]
        if isinstance(self.upsample_net, upsample.ConvInUpsampleNetwork):
            c = self.upsample_net.stream_forward(c, up_in, up_out, precision)
        else:
            c = self.upsample_net.stream_forward(c, up_in, up_out)  # (stretch stages only: fp32 in either precision)
        assert c.size(-1) == z.size(-1)
        x = stream_pointwise(self.first_conv, z, precision)
        skips = None
        for i, (f, (h_in, h_out)) in enumerate(zip(self.conv_layers, hist[n_up:])):
            x, skips = f.stream_forward(x, c, h_in, h_out, skips=skips,
                                        skip_scale=math.sqrt(1.0 / n) if i == n - 1 else 1.0, inplace_skips=True,
                                        precision=precision)
        x = stream_pointwise(self.last_conv_layers[1], skips, precision, pre_act="relu")
        return stream_pointwise(self.last_conv_layers[3], x, precision, pre_act="relu")

    # ---- streaming the NON-causal generator with a fixed look-ahead (utils.PWGLookaheadStream)
    def lookahead_unsupported_reason(self, batch=1, precision="fp32"):
        """None if the non-causal generator streams with a look-ahead in ``precision``, else the reason (host logic
        only)."""
        if any(f.use_causal_conv for f in self.conv_layers):
            return ("the model is causal (use_causal_conv=True) and streams without look-ahead through utils.PWGStream")
        if self.upsample_net is None:
            return "upsample_conditional_features=False: the stream maps mel frames to samples through the upsampler"
        if not isinstance(self.upsample_net, (upsample.UpsampleNetwork, upsample.ConvInUpsampleNetwork)):
            return (f"upsample_net={self.upsample_net.__class__.__name__!r} is not built for streams (only UpsampleNetwork "
                    "and ConvInUpsampleNetwork)")
        net = self.upsample_net.upsample if isinstance(self.upsample_net, upsample.ConvInUpsampleNetwork) \
            else self.upsample_net
        reason = net.lookahead_unsupported_reason()
        if reason is not None:
            return "the mel upsampler: " + reason
        c_delay = 0
        for f in self.conv_layers:
            c_delay += f.conv.dilation
            reason = f.lookahead_unsupported_reason(batch, 8, c_delay, precision)
            if reason is not None:
                return f"{f.__class__.__name__}: {reason}"
        return None

    def lookahead_plan(self):
        """Every launch of one push of the look-ahead stream, in the order :meth:`lookahead_forward` runs them, as
        ``PWGLookaheadLaunch(kind, module, rate, delay, c_delay, state)``: output columns per mel frame, delay of the
        output in columns, how late a gated layer reads the conditioning, and the ``(channels, columns)`` of the state
        tensors it keeps.  ``conv_in`` (delay ``w`` frames), the upsampling stages (``D * s + s``), the noise line and
        ``first_conv`` (the conditioning's delay ``D_c``), the conditioning line (``sum d`` columns), the gated layers
        (``+ d`` each: history ``2 d``, from the second on a skip line of ``d``) and the two last 1 x 1 convolutions.
        The last launch's delay is the stream's latency in samples.  Pure host logic; ValueError with the reason for a
        generator that does not stream this way."""
        from ..layers.causal_conv import PWGLookaheadLaunch as Launch

        reason = self.lookahead_unsupported_reason()
        if reason is not None:
            raise ValueError(f"{self.__class__.__name__}: {reason}")
        if isinstance(self.upsample_net, upsample.ConvInUpsampleNetwork):
            plan, delay, rate = self.upsample_net.lookahead_plan()
        else:
            plan, delay, rate = self.upsample_net.lookahead_plan(self.aux_channels)
        plan = list(plan)
        plan.append(Launch("noise", None, rate, delay, 0, [(self.in_channels, delay)] if delay else []))
        plan.append(Launch("first_conv", self.first_conv, rate, delay, 0, []))
        reach = sum(f.conv.dilation for f in self.conv_layers)
        plan.append(Launch("cond_line", None, rate, delay, 0, [(self.aux_channels, reach)]))
        c_delay = 0
        for i, f in enumerate(self.conv_layers):
            d = f.conv.dilation
            c_delay, delay = c_delay + d, delay + d
            state = [(f.conv.in_channels, (f.conv.kernel_size - 1) * d)]
            if i > 0:
                state.append((f.conv1x1_skip.out_channels, d))
            plan.append(Launch("layer", f, rate, delay, c_delay, state))
        for cv in (self.last_conv_layers[1], self.last_conv_layers[3]):
            plan.append(Launch("last_conv", cv, rate, delay, 0, []))
        return plan

    @torch.no_grad()
    def lookahead_forward(self, z, c, walk):
        """The NON-causal ``forward`` on the next chunk of a look-ahead stream: noise z (B, 1, n * upsample_factor) for the
        samples of the mel frames c (B, C, n), undelayed -> (B, out_channels, n * upsample_factor), late by the plan's
        last delay.  ``walk``: a :class:`layers.causal_conv.PWGLookaheadWalk` over :meth:`lookahead_plan`.  Every layer
        runs in its causal form on a shifted time axis: the noise waits for the conditioning in a delay line, every gated
        layer reads the conditioning from the shared line at its own delay and the running skip sum through its skip
        line, and every launch stores zeros outside the utterance.  The last block applies sqrt(1 / layers).  The walk's
        ``precision`` is the push's: ``"bf16"`` runs ``conv_in``, the 1 x 1 convolutions and the gated layers with bf16
        operands; the stretch stages, the delay lines and every state tensor stay fp32."""
        from ..layers.causal_conv import lookahead_line, lookahead_pointwise

        frames, precision = c.shape[-1], walk.precision
        if isinstance(self.upsample_net, upsample.ConvInUpsampleNetwork):
            c = self.upsample_net.lookahead_forward(c, walk)
        else:
            c = self.upsample_net.lookahead_forward(c, walk, frames)
        assert c.size(-1) == z.size(-1)
        _, pairs, where = walk.take("noise", None, frames)
        if pairs:
            z = lookahead_line(z, pairs[0], where, delayed=True)
        _, _, valid = walk.take("first_conv", self.first_conv, frames)
        x = lookahead_pointwise(self.first_conv, z, valid, precision)
        _, ((c_line, c_line_out),), where = walk.take("cond_line", None, frames)
        lookahead_line(c, (c_line, c_line_out), where)
        skips, n = None, len(self.conv_layers)
        for i, f in enumerate(self.conv_layers):
            launch, pairs, valid = walk.take("layer", f, frames)
            x, skips = f.lookahead_forward(x, c, c_line, launch.c_delay, pairs[0], skips,
                                           pairs[1] if i > 0 else (None, None), valid,
                                           skip_scale=math.sqrt(1.0 / n) if i == n - 1 else 1.0, precision=precision)
        _, _, valid = walk.take("last_conv", self.last_conv_layers[1], frames)
        x = lookahead_pointwise(self.last_conv_layers[1], skips, valid, precision, pre_act="relu")
        _, _, valid = walk.take("last_conv", self.last_conv_layers[3], frames)
        return lookahead_pointwise(self.last_conv_layers[3], x, valid, precision, pre_act="relu")

    @staticmethod
    def _get_receptive_field_size(layers, stacks, kernel_size, dilation=lambda x: 2 ** x):
        assert layers % stacks == 0
        per_cycle = layers // stacks
        return (kernel_size - 1) * sum(dilation(i % per_cycle) for i in range(layers)) + 1

    @property
    def receptive_field_size(self):
        return self._get_receptive_field_size(self.layers, self.stacks, self.kernel_size)

    def register_stats(self, stats):
        from ..utils import load_stats

        mean, scale = load_stats(stats)
        self.register_buffer("mean", torch.from_numpy(mean).float())
        self.register_buffer("scale", torch.from_numpy(scale).float())
        logging.info("Successfully registered stats as buffer.")

    def inference(self, c=None, x=None, normalize_before=False, precision=None):
        """c: (T', C) mel, x: (T, 1) noise (drawn here if omitted) -> (T, out_channels).

        ``precision``: None = whatever ``utils.set_inference_precision`` set on the model (default fp32); ``"bf16"`` /
        ``"fp32"`` = this call only (the modules' settings are restored afterwards).  A bf16 call runs under
        ``torch.no_grad()``: the mode has no backward pass."""
        from ..utils.precision import inference_precision, no_grad_if_bf16

        with inference_precision(self, precision), no_grad_if_bf16(self):
            return self._inference(c, x, normalize_before)

    def _inference(self, c, x, normalize_before):
        dev = next(self.parameters()).device
        if x is not None:
            if not isinstance(x, torch.Tensor):
                x = torch.tensor(x, dtype=torch.float).to(dev)
            x = x.transpose(1, 0).unsqueeze(0).contiguous()
        else:
            assert c is not None
            x = torch.randn(1, 1, len(c) * self.upsample_factor).to(dev)
        if c is not None:
            if not isinstance(c, torch.Tensor):
                c = torch.tensor(c, dtype=torch.float).to(dev)
            if normalize_before:
                c = (c - self.mean) / self.scale
            c = c.transpose(1, 0).unsqueeze(0).contiguous()
            c = Fn.pad1d(c, self.aux_context_window, self.aux_context_window, "replicate")
        return self.forward(x, c).squeeze(0).transpose(1, 0)


class ParallelWaveGANDiscriminator(torch.nn.Module, _WeightNormMixin):
    """Dilated conv stack discriminator (reference: models/parallel_wavegan.py:264-371)."""

    def __init__(self, in_channels=1, out_channels=1, kernel_size=3, layers=10, conv_channels=64, dilation_factor=1,
                 nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.2}, bias=True,
                 use_weight_norm=True):
        super().__init__()
        assert (kernel_size - 1) % 2 == 0, "Not support even number kernel size."
        assert dilation_factor > 0, "Dilation factor must be > 0."
        self.conv_layers = torch.nn.ModuleList()
        conv_in_channels = in_channels
        for i in range(layers - 1):
            if i == 0:
                dilation = 1
            else:
                dilation = i if dilation_factor == 1 else dilation_factor ** i
                conv_in_channels = conv_channels
            self.conv_layers.append(Conv1d(conv_in_channels, conv_channels, kernel_size=kernel_size,
                                           padding=(kernel_size - 1) // 2 * dilation, dilation=dilation, bias=bias))
            self.conv_layers.append(FusedActivation(nonlinear_activation, **nonlinear_activation_params))
        self.conv_layers.append(Conv1d(conv_in_channels, out_channels, kernel_size=kernel_size,
                                       padding=(kernel_size - 1) // 2, bias=bias))
        if use_weight_norm:
            self.apply_weight_norm()

    def forward(self, x):
        """(B, 1, T) -> (B, 1, T)."""
        # each LeakyReLU rides on the NEXT convolution as its pre-activation (applied to the staged input tile), so
        # that the backward needs no separate activation-gradient pass: the next convolution's data-gradient kernel
        # multiplies by act'(x) in its epilogue and its weight-gradient kernel re-applies act on load.
        pending = None
        for mod in self.conv_layers:
            if isinstance(mod, FusedActivation):
                pending = mod
                continue
            if pending is None:
                x = mod(x)
            else:
                x = mod(x, pre_act=pending.kind, pre_slope=pending.slope)
            pending = None
        if pending is not None:
            raise RuntimeError("ParallelWaveGANDiscriminator: the layer list must end with a convolution")
        return x


class ResidualParallelWaveGANDiscriminator(torch.nn.Module, _WeightNormMixin):
    """WaveNet-style discriminator (reference: models/parallel_wavegan.py:374-513): 1x1 conv +
    LeakyReLU, ``layers`` gated residual blocks without conditioning, skip sum * sqrt(1/layers),
    LeakyReLU, 1x1, LeakyReLU, 1x1.  Activations, the running skip sum and its scale ride on the
    convolution kernels' epilogues exactly as in the generator."""

    def __init__(self, in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=64,
                 gate_channels=128, skip_channels=64, dropout=0.0, bias=True, use_weight_norm=True,
                 use_causal_conv=False, nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.2}):
        super().__init__()
        assert (kernel_size - 1) % 2 == 0, "Not support even number kernel size."
        self.in_channels, self.out_channels = in_channels, out_channels
        self.layers, self.stacks, self.kernel_size = layers, stacks, kernel_size
        assert layers % stacks == 0
        layers_per_stack = layers // stacks

        def act():
            return FusedActivation(nonlinear_activation, **nonlinear_activation_params)

        self.first_conv = torch.nn.Sequential(Conv1d1x1(in_channels, residual_channels, bias=True), act())
        self.conv_layers = torch.nn.ModuleList()
        for layer in range(layers):
            self.conv_layers.append(ResidualBlock(
                kernel_size=kernel_size, residual_channels=residual_channels, gate_channels=gate_channels,
                skip_channels=skip_channels, aux_channels=-1, dilation=2 ** (layer % layers_per_stack),
                dropout=dropout, bias=bias, use_causal_conv=use_causal_conv))
        self.last_conv_layers = torch.nn.ModuleList([
            act(), Conv1d1x1(skip_channels, skip_channels, bias=True), act(),
            Conv1d1x1(skip_channels, out_channels, bias=True)])
        if use_weight_norm:
            self.apply_weight_norm()

    def forward(self, x):
        """(B, 1, T) -> (B, 1, T)."""
        a0 = self.first_conv[1]
        x = self.first_conv[0](x, post_act=a0.kind, post_slope=a0.slope)
        skips = None
        n = len(self.conv_layers)
        for i, f in enumerate(self.conv_layers):
            x, skips = f(x, None, skips=skips, skip_scale=math.sqrt(1.0 / n) if i == n - 1 else 1.0)
        a1, c1, a2, c2 = self.last_conv_layers
        x = c1(skips, pre_act=a1.kind, pre_slope=a1.slope)
        return c2(x, pre_act=a2.kind, pre_slope=a2.slope)
