"""MelGAN residual stack (drop-in for parallel_wavegan.layers.residual_stack)."""
import os

import torch

from .. import functional as Fn
from .. import ops
from .activation import FusedActivation
from .causal_conv import CausalConv1d, LookaheadLaunch, lookahead_delay, mirrored_delay
from .conv import Conv1d, group_image
from .padding import FusedPad, get_pad


class ResidualStack(torch.nn.Module):
    """``[act, pad(d), conv k3 dil d, act, conv 1x1](c) + skip 1x1(c)`` (layers/residual_stack.py:13-85).
    MelGAN's geometries (48 / 96 / 192 channels, kernel 3, reflect padding, LeakyReLU) run as ONE launch
    (csrc/resstack.hip; ``fuse_unit``); everything else as three: skip conv; dilated conv with activation + reflect
    padding fused on its input; 1x1 conv with activation fused on its input and the skip branch fused as addend."""

    fuse_unit = os.environ.get("PWG_RESSTACK", "1") != "0"  # (0: the three-launch path, for A/B measurements)
    # backward of the unit: its data gradient as one launch (functional.ResStackFn) instead of the three layers' own
    fuse_unit_backward = os.environ.get("PWG_RESSTACK_BWD", "1") != "0"

    def __init__(self, kernel_size=3, channels=32, dilation=1, bias=True, nonlinear_activation="LeakyReLU",
                 nonlinear_activation_params={"negative_slope": 0.2}, pad="ReflectionPad1d", pad_params={},
                 use_causal_conv=False):
        super().__init__()
        self.use_causal_conv = use_causal_conv
        if use_causal_conv:
            # layers/residual_stack.py:56-69 of the reference: no separate pad module, hence 4 entries
            self.stack = torch.nn.Sequential(
                FusedActivation(nonlinear_activation, **nonlinear_activation_params),
                CausalConv1d(channels, channels, kernel_size, dilation=dilation, bias=bias, pad=pad,
                             pad_params=pad_params),
                FusedActivation(nonlinear_activation, **nonlinear_activation_params),
                Conv1d(channels, channels, 1, bias=bias),
            )
        else:
            assert (kernel_size - 1) % 2 == 0, "Not support even number kernel size."
            p = (kernel_size - 1) // 2 * dilation
            padm = get_pad(pad, p, **pad_params)
            self.stack = torch.nn.Sequential(
                FusedActivation(nonlinear_activation, **nonlinear_activation_params),
                padm,
                Conv1d(channels, channels, kernel_size, dilation=dilation, bias=bias, padding=p, pad_mode=padm.mode),
                FusedActivation(nonlinear_activation, **nonlinear_activation_params),
                Conv1d(channels, channels, 1, bias=bias),
            )
        self.skip_layer = Conv1d(channels, channels, 1, bias=bias)
        if (self.fuse_unit and not use_causal_conv and kernel_size == 3 and channels in (48, 96, 192) and dilation <= 27
                and padm.mode == "reflect" and self.stack[0].kind == "leaky_relu" and 0.0 < self.stack[0].slope < 1.0):
            # the geometries the one-launch unit covers (csrc/resstack.hip): the unit packs its own image of the three
            # weights, so the weight bank prepares only their row scales; a call the unit turns down at run time
            # (T % 4 != 0, a non-contiguous input) packs the layers' images lazily
            for cv in self.unit_convs():
                cv.bank_images = False

    def parts(self):
        """``(act0, conv0, act1, conv1, skip)``: activation and dilated convolution, activation and 1 x 1 convolution, the
        skip 1 x 1 -- in either layout (the causal ``stack`` has no pad module, hence other indices).  One pass over the
        ``Sequential``: indexing it is several times slower, and a stream's push is host-bound."""
        a0, conv0, a1, conv1 = (m for m in self.stack if not isinstance(m, FusedPad))
        return a0, conv0, a1, conv1, self.skip_layer

    def unit_convs(self):
        """(dilated convolution, 1x1 convolution, skip 1x1)."""
        _, conv0, _, conv1, skip = self.parts()
        return conv0, conv1, skip

    def unit_slope(self):
        return self.stack[0].slope

    def unit_params(self):
        """Parameters in the order functional.ResStackFn returns their gradients."""
        ps = []
        for cv in self.unit_convs():
            ps.append(cv.raw_weight)
            if cv.has_weight_norm:
                ps.append(cv.weight_g)
            if cv.bias is not None:
                ps.append(cv.bias)
        return ps

    def unit_image(self):
        """MFMA A-operand image of the three weights for the current parameter values (cached)."""
        return group_image(self, "_unit_img", self.unit_convs(), ops.resstack_pack_weight)

    def unit_image_bwd(self):
        """The same for the unit's data gradient (transposed weights)."""
        return group_image(self, "_unit_img_bwd", self.unit_convs(), ops.resstack_pack_weight_bwd)

    def _unit_modules_ok(self):
        """What the one-launch unit (csrc/resstack.hip) asks of the modules, whatever the input."""
        if not self.fuse_unit or self.use_causal_conv:
            return False
        a0, conv0, a1, conv1, skip = self.parts()
        if any(cv.has_spectral_norm or cv.groups != 1 or cv.stride != 1 for cv in (conv0, conv1, skip)):
            return False
        if (conv0.kernel_size != 3 or conv0.pad_mode != "reflect" or conv0.padding != conv0.dilation
                or conv0.padding_right != conv0.dilation or conv1.kernel_size != 1 or skip.kernel_size != 1):
            return False
        if a0.kind != "leaky_relu" or a1.kind != "leaky_relu" or a0.slope != a1.slope or not 0.0 < a0.slope < 1.0:
            return False
        ch = conv0.in_channels
        return all(cv.in_channels == ch and cv.out_channels == ch for cv in (conv0, conv1, skip))

    def _unit_ok(self, c):
        if not c.is_cuda or c.dim() != 3 or c.dtype != torch.float32 or not self._unit_modules_ok():
            return False
        conv0 = self.parts()[1]
        # (rows are staged with 16-B LDS-DMA pieces; 4-B source alignment is enough)
        if c.shape[1] != conv0.in_channels or not c.is_contiguous():
            return False
        return ops.resstack_supported(conv0.in_channels, c.shape[2], conv0.dilation)

    def forward(self, c):
        a0, conv0, a1, conv1, skip_layer = self.parts()
        if self._unit_ok(c):
            convs = (conv0, conv1, skip_layer)
            bias = [None if cv.bias is None else cv.bias.detach() for cv in convs]
            needs_grad = torch.is_grad_enabled() and (c.requires_grad or any(p.requires_grad for p in self.parameters()))
            if needs_grad and self.fuse_unit_backward:
                return Fn.ResStackFn.apply(c, self, *self.unit_params())
            with torch.no_grad():
                y, h = ops.resstack_forward(c, self.unit_image(), conv0.dilation, a0.slope, *bias, save_h=needs_grad)
            if not needs_grad:
                return y
            # the three layers' autograd nodes, without their launches: the values come from the one-launch unit, the
            # backward pass is the layers' own (the skip branch's value is never read: only its gradient path matters)
            skip = skip_layer(c, precomputed=torch.empty_like(y))
            t = conv0(c, pre_act=a0.kind, pre_slope=a0.slope, precomputed=h)
            return conv1(t, pre_act=a1.kind, pre_slope=a1.slope, add1=skip, precomputed=y)
        skip = skip_layer(c)
        t = conv0(c, pre_act=a0.kind, pre_slope=a0.slope)
        return conv1(t, pre_act=a1.kind, pre_slope=a1.slope, add1=skip)

    # ---- utterances of different lengths in one batch (MelGANGenerator.forward_ragged)
    def ragged_fuses(self, rate):
        """Does :meth:`forward_ragged` run this stack as the ragged form of the one-launch unit at ``rate`` columns per
        frame, for every batch of at least 64 columns?  Pure host logic over the module geometry (``_unit_modules_ok``,
        and ``ops.resstack_ragged_supported`` at a covered length)."""
        conv0 = self.parts()[1]
        return self._unit_modules_ok() and ops.resstack_ragged_supported(conv0.in_channels, 64, conv0.dilation, rate)

    @torch.no_grad()
    def forward_ragged(self, x, frames, rate):
        """``forward`` over a ragged batch (inference): ``frames`` is the device int32 table of frames per
        item, ``rate`` the columns of ``x`` per frame; item ``b`` is the sequence ``[0, frames[b] * rate)`` of its rows and
        the reflection mirrors at its end.  Returns ``(y, tail)``: ``tail`` is 0 when ``y`` holds exact zeros past every
        item's end and None when it holds unspecified values there.

        Where :meth:`ragged_fuses` the stack is ONE launch of the ragged unit (csrc/resstack.hip): it reads nothing
        past an item's end, so ``x`` may hold anything there, and it stores zeros there (``tail`` 0).  Otherwise the three
        launches of ``forward``: ``ops.mirror_tail`` first writes the dilated convolution's ``dilation`` mirror columns
        behind every item IN PLACE into ``x`` (the caller's intermediate; the columns must fit inside the buffer, the
        slack rule of ``MelGANGenerator.forward_ragged``); ``tail`` None."""
        if self.use_causal_conv:
            raise ValueError("ResidualStack: a causal stack has no ragged forward (it streams: stream_forward)")
        a0, conv0, a1, conv1, skip_layer = self.parts()
        if conv0.pad_mode != "reflect":
            raise ValueError(f"ResidualStack: pad = {self.stack[1].__class__.__name__}; only a ReflectionPad1d stack has "
                             "a ragged forward (ops.mirror_tail writes the mirror of every item's own end)")
        ops._require_device(x)
        x = x.contiguous()
        if self.ragged_fuses(rate):
            if not ops.resstack_ragged_supported(x.shape[1], x.shape[2], conv0.dilation, rate):
                raise ValueError(f"ResidualStack.forward_ragged: {x.shape[2]} columns per item; the one-launch unit covers "
                                 "64 columns and more (below 4 GB per item): pad the batch")
            bias = [None if cv.bias is None else cv.bias.detach() for cv in (conv0, conv1, skip_layer)]
            return ops.resstack_forward_ragged(x, frames, rate, self.unit_image(), conv0.dilation, a0.slope, *bias), 0
        ops.mirror_tail(x, frames, rate, conv0.padding)
        skip = skip_layer(x)
        t = conv0(x, pre_act=a0.kind, pre_slope=a0.slope)
        return conv1(t, pre_act=a1.kind, pre_slope=a1.slope, add1=skip), None

    def stream_layers(self):
        """The causal convolutions that keep history (the 1 x 1 layers have none)."""
        return [self.stack[1]]

    # ---- the NON-causal stack streamed with a fixed look-ahead (utils.MelGANLookaheadStream)
    def lookahead_plan(self, delay_in, rate):
        """Delay plan of the non-causal stack on an input delayed by ``delay_in`` columns -> ``(launches, delay_out)``:
        the skip 1 x 1 at the input's delay, the reflect-padded dilated convolution (the mirrored form), which adds its
        padding, and the second 1 x 1 with the skip as addend 1 through a delay line of that padding.  ValueError for a
        causal stack and for a layer without such a form."""
        if self.use_causal_conv:
            raise ValueError("ResidualStack: a causal stack streams without look-ahead (utils.CausalStream)")
        conv0, conv1, skip = self.unit_convs()
        d_skip = lookahead_delay(skip, delay_in)
        d0 = mirrored_delay(conv0, delay_in)
        d1 = lookahead_delay(conv1, d0)
        return [LookaheadLaunch(skip, rate, d_skip, 0, 0), LookaheadLaunch(conv0, rate, d0, 0, 0),
                LookaheadLaunch(conv1, rate, d1, d1 - d_skip, 0)], d1

    def walk_forward(self, c, walk):
        """``forward`` on the next chunk of a stream, three launches through ``walk``.  A
        :class:`layers.causal_conv.CausalWalk`: the causal stack; the skip and second 1 x 1 convolutions keep no history,
        but they too run on the streaming kernel (``H = 0``): the general kernel picks its tile and its split of the
        reduction from the column count and the batch, so its sums would depend on how the stream is cut into pushes.  A
        ``LookaheadWalk`` / ``SlotWalk``: the launches of :meth:`lookahead_plan`, the walk delaying the skip."""
        a0, conv0, a1, conv1, skip_layer = self.parts()
        skip = walk.run(skip_layer, c)
        t = walk.run(conv0, c, pre_act=a0.kind, pre_slope=a0.slope)
        return walk.run(conv1, t, add1=skip, pre_act=a1.kind, pre_slope=a1.slope)
