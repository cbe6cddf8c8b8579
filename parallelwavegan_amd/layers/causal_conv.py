"""Causal convolution modules (drop-in for parallel_wavegan.layers.causal_conv).

Same constructor arguments, sub-module names (``pad`` / ``conv`` / ``deconv``) and hence state-dict
keys as the reference (/root/reference/parallel_wavegan/layers/causal_conv.py:12-77).  No tensor is
padded and trimmed: a causal convolution is the MFMA convolution kernel with left-only padding
``(k-1)*d`` and ``t_out = t_in``; the causal transposed convolution is the polyphase kernel with
``padding = stride`` (which is exactly the reference's ``[stride:-stride]`` trim) on an input that
got one replicated sample on the left.
"""
import collections

import torch

from .. import functional as Fn
from .. import ops
from .conv import Conv1d, ConvTranspose1d
from .padding import get_pad


class CausalConv1d(torch.nn.Module):
    """``conv(pad_left(x, (k-1)*d))[:, :, :T]`` (causal_conv.py:12-43) as one launch."""

    def __init__(self, in_channels, out_channels, kernel_size, dilation=1, bias=True, pad="ConstantPad1d",
                 pad_params={"value": 0.0}):
        super().__init__()
        p = (kernel_size - 1) * dilation
        self.pad = get_pad(pad, p, **pad_params)  # marker (no parameters); the kernel pads implicitly
        self.conv = Conv1d(in_channels, out_channels, kernel_size, dilation=dilation, bias=bias, padding=(p, 0),
                           pad_mode=self.pad.mode)

    def forward(self, x, **fused):
        """Accepts the fused-epilogue keywords of :class:`Conv1d` (pre_act, add1, post_act, ...)."""
        return self.conv(x, **fused)

    def stream_desc(self, batch, n, **fused):
        """Descriptor of one push of ``n`` columns through the streaming kernel (csrc/conv1d_stream.hip)."""
        cv = self.conv
        return ops.make_conv_desc(batch, cv.in_channels, cv.out_channels, n, n, cv.kernel_size, 1, cv.dilation, cv.padding,
                                  cv.groups, transposed=False, pad_mode=cv.pad_mode, **fused)

    def history_shape(self, batch):
        """Shape of one history buffer: the last ``(k - 1) * d`` raw input columns (allocate two: ping-pong)."""
        return (batch, self.conv.in_channels, self.conv.padding)

    def history_columns_at_start(self):
        """Input columns the first push needs: reflect padding mirrors the first ``(k - 1) * d + 1`` of them."""
        return self.conv.padding + 1 if self.conv.pad_mode == "reflect" and self.conv.padding > 0 else 1

    def stream_forward(self, x, hist_in, hist_out, precision="fp32", **fused):
        """The next ``x.shape[-1]`` columns of a stream whose previous columns are ``hist_in`` (None: start of stream,
        the layer's own padding); also writes ``hist_out`` (a buffer distinct from ``hist_in``).  One launch; the
        fused-epilogue keywords and the weight image are those of ``forward``.  ``precision="bf16"``: the same launch
        with bf16 operands (csrc/conv1d_stream_bf16.hip) on the layer's bf16 image; history stays raw fp32, so the
        state of a stream does not depend on its precision."""
        return _stream_forward(self.conv, self.stream_desc(x.shape[0], x.shape[-1], **_desc_kw(fused)), x, hist_in,
                               hist_out, fused, precision)


class CausalConvTranspose1d(torch.nn.Module):
    """``deconv(replicate_pad_left(x, 1))[:, :, stride:-stride]`` (causal_conv.py:46-77)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, bias=True, pad="ReplicationPad1d",
                 pad_params={}):
        super().__init__()
        self.pad = get_pad(pad, 1, **pad_params)
        if self.pad.mode == "zero" and getattr(self.pad, "value", 0.0) != 0.0:
            raise NotImplementedError("CausalConvTranspose1d: constant padding with a non-zero value")
        # ConvTranspose1d(padding=stride) == full transposed convolution trimmed by `stride` on both sides
        self.deconv = ConvTranspose1d(in_channels, out_channels, kernel_size, stride, padding=stride, bias=bias)
        self.stride = stride

    def forward(self, x, **fused):
        # the left pad and an element-wise pre-activation commute, so the activation stays fused
        return self.deconv(Fn.pad1d(x, 1, 0, self.pad.mode), **fused)

    def stream_desc(self, batch, n, **fused):
        """Descriptor of one push of ``n`` columns (``n * stride`` out) through the streaming kernel."""
        cv = self.deconv
        return ops.make_conv_desc(batch, cv.in_channels, cv.out_channels, n, n * self.stride, cv.kernel_size, self.stride, 1,
                                  cv.padding, cv.groups, transposed=True, pad_mode=self.pad.mode, **fused)

    def history_shape(self, batch):
        """Shape of one history buffer: the previous raw input column (allocate two: ping-pong)."""
        return (batch, self.deconv.in_channels, 1)

    def history_columns_at_start(self):
        return 1

    def stream_forward(self, x, hist_in, hist_out, precision="fp32", **fused):
        """As :meth:`CausalConv1d.stream_forward`; the start-of-stream context is the replicated first column."""
        return _stream_forward(self.deconv, self.stream_desc(x.shape[0], x.shape[-1], **_desc_kw(fused)), x, hist_in,
                               hist_out, fused, precision)


def stream_pointwise(cv, x, precision="fp32", **fused):
    """A 1 x 1 ``Conv1d`` on the next columns of a stream, through the streaming kernel with no history (``H = 0``):
    its sum order does not depend on the column count or the batch, which the general kernel's choice of tile and
    reduction split does.  ``precision`` as in :meth:`CausalConv1d.stream_forward`."""
    if cv.kernel_size != 1 or cv.padding != 0 or cv.padding_right != 0:
        raise ValueError("stream_pointwise: not an unpadded 1 x 1 convolution")
    return _stream_forward(cv, pointwise_desc(cv, x.shape[0], x.shape[-1], **_desc_kw(fused)), x, None, None, fused,
                           precision)


class CausalWalk:
    """The walk of a CAUSAL model's ``stream_layers()`` (utils.CausalStream): ``run`` has the contract of
    :meth:`LookaheadWalk.run`, so a module runs its convolutions through either with one loop.  ``hist_in`` (None: start
    of stream, every layer's own padding) / ``hist_out``: one history tensor per layer, a ping-pong half each -- a list of
    the wrong length is an error, not a shorter walk; ``precision``: of every launch of the push."""

    def __init__(self, layers, hist_in, hist_out, precision="fp32"):
        n = len(layers)
        if len(hist_out) != n or (hist_in is not None and len(hist_in) != n):
            raise ValueError(f"stream_forward: hist_in / hist_out hold {None if hist_in is None else len(hist_in)} / "
                             f"{len(hist_out)} history tensors, stream_layers() has {n}")
        self.precision = precision
        self._layers = iter(layers)
        self._pairs = iter(zip(hist_in if hist_in is not None else [None] * n, hist_out))

    def take(self, layer):
        """The ``(hist_in, hist_out)`` pair of the next layer of ``stream_layers()``, which must be ``layer``."""
        expected, _ = next(self._layers, (None, None))
        if expected is not layer:
            raise RuntimeError(f"causal walk out of step: stream_layers() expects {expected}, the model ran {layer}")
        return next(self._pairs)

    def run(self, cv, x, add1=None, add2=None, **fused):
        """``cv`` on the chunk ``x``, one launch; fused-epilogue keywords as in ``forward``.  A causal convolution must be
        the next layer of ``stream_layers()`` and takes its history pair; an unpadded 1 x 1 ``Conv1d`` keeps no state."""
        if isinstance(cv, (CausalConv1d, CausalConvTranspose1d)):
            return cv.stream_forward(x, *self.take(cv), precision=self.precision, add1=add1, add2=add2, **fused)
        return stream_pointwise(cv, x, precision=self.precision, add1=add1, add2=add2, **fused)


def _desc_kw(fused):
    return {k: v for k, v in fused.items() if k not in ("add1", "add2")}


# ---- the rule of a stream launch, stated once.  A form's row per precision: the kernel's name in a
# refusal, the coverage query, the launch.  A (form, precision) without a row does not exist yet.
_STREAM_KERNELS = {
    ("plain", "fp32"): ("streaming kernel", ops.conv1d_stream_supported, ops.conv1d_stream_forward),
    ("plain", "bf16"): ("bf16 streaming kernel", ops.conv1d_stream_bf16_supported, ops.conv1d_stream_forward_bf16),
    ("delayed", "fp32"): ("delayed streaming kernel", ops.conv1d_stream_delayed_supported,
                          ops.conv1d_stream_delayed_forward),
    ("delayed", "bf16"): ("delayed bf16 streaming kernel", ops.conv1d_stream_bf16_delayed_supported,
                          ops.conv1d_stream_delayed_forward_bf16),
    ("mirrored", "fp32"): ("mirrored streaming kernel", ops.conv1d_stream_mirrored_supported,
                           ops.conv1d_stream_mirrored_forward),
    # (the slotted form has no query of its own: its coverage is the delayed form's)
    ("slots", "fp32"): ("slotted streaming kernel", ops.conv1d_stream_delayed_supported, ops.conv1d_stream_slots_forward),
    ("slots", "bf16"): ("slotted bf16 streaming kernel", ops.conv1d_stream_bf16_delayed_supported,
                        ops.conv1d_stream_slots_forward_bf16),
    # (nor has the slotted-mirrored form: its coverage is the mirrored form's)
    ("slots_mirrored", "fp32"): ("slotted mirrored streaming kernel", ops.conv1d_stream_mirrored_supported,
                                 ops.conv1d_stream_slots_mirrored_forward),
}
# what an fp32 launch tells a module in bf16 mode, per form
_LOOKAHEAD_IS_FP32 = ("the look-ahead stream is fp32 (utils.set_inference_precision(model, 'fp32'), or pass "
                      "precision='bf16' to stream with bf16 operands)")
_FORM_IS_FP32 = {"plain": "the streaming kernel is fp32 (pass precision='bf16' to stream with bf16 operands)",
                 "delayed": _LOOKAHEAD_IS_FP32, "mirrored": _LOOKAHEAD_IS_FP32, "slots": _LOOKAHEAD_IS_FP32,
                 "slots_mirrored": _LOOKAHEAD_IS_FP32}
_FORM_IS_FP32_ONLY = {"mirrored": "a reflect-padded layer streams with a look-ahead in fp32 only",
                      "slots_mirrored": "a reflect-padded layer streams with a look-ahead in fp32 only"}


def _launch(form, precision, cv, desc, x, hist, *args, delays=(), **kwargs):
    """One launch of ``cv`` under ``desc`` through the ``form`` (a key of ``_STREAM_KERNELS``) of the streaming kernel
    on the chunk ``x`` and the history pair ``hist``; ``args`` / ``kwargs``: what the form's launch takes behind the
    bias (addends, delay lines, windows), ``delays``: what its coverage query takes behind the descriptor.  The
    precision is the call's: a bf16 call does not consult the module's own ``precision`` attribute (whole-utterance mode)
    and runs on the layer's bf16 image; an fp32 call refuses a module in bf16 mode.  A layer the kernel does not cover is
    a RuntimeError that names the reason."""
    if precision not in ("fp32", "bf16"):
        raise ValueError(f"stream precision must be 'fp32' or 'bf16', got {precision!r}")
    if precision == "fp32" and cv.precision != "fp32":
        raise RuntimeError(f"{cv.__class__.__name__} is in {cv.precision} inference precision: {_FORM_IS_FP32[form]}")
    if (form, precision) not in _STREAM_KERNELS:
        raise RuntimeError(f"the {form} form of the streaming kernel has no {precision} form yet: "
                           + _FORM_IS_FP32_ONLY[form])
    kernel, supported, forward = _STREAM_KERNELS[form, precision]
    if not supported(desc, *delays):
        from .. import _lib

        raise RuntimeError(f"the {kernel} does not cover this layer: "
                           + _lib.lib().pwg_last_error().decode(errors="replace"))
    bias = None if cv.bias is None else cv.bias.detach()
    with torch.no_grad():
        image = cv.packed_weight_bf16() if precision == "bf16" else cv.packed_weight()
        return forward(desc, x.contiguous(), hist[0], hist[1], image, bias, *args, **kwargs)


def _stream_forward(cv, desc, x, hist_in, hist_out, fused, precision="fp32"):
    return _launch("plain", precision, cv, desc, x, (hist_in, hist_out), fused.get("add1"), fused.get("add2"))


# ---- the NON-causal layers in causal form: streaming with a fixed look-ahead (utils.LookaheadStream).
# A symmetric ``Conv1d(k, d, padding (k-1)d/2)`` is its causal form (history ``(k-1)d``) on a time axis shifted by its
# padding; a ``ConvTranspose1d(2s, s, padding s//2 + s%2)`` is the causal polyphase form (one column of history, zero
# start) shifted by its padding.  Every tensor of the streamed network therefore has a delay: stream column ``t`` holds
# the whole-utterance column ``t - delay``, and exact zeros where that column does not exist.

def lookahead_delay(cv, delay_in):
    """Delay (columns) of the output of the non-causal ``cv`` run in causal form on an input delayed by ``delay_in``.
    ValueError for a layer that has no such form."""
    if cv.groups != 1 or cv.pad_mode != "zero":
        raise ValueError(f"{cv}: only zero-padded, ungrouped layers stream with a look-ahead")
    if cv.transposed:
        s = cv.stride
        if cv.kernel_size != 2 * s or cv.padding != s // 2 + s % 2 or cv.output_padding != s % 2 or cv.dilation != 1:
            raise ValueError(f"{cv}: only ConvTranspose1d(kernel 2s, stride s, padding s//2 + s%2, output_padding s%2) "
                             "streams with a look-ahead")
        return delay_in * s + cv.padding
    reach = (cv.kernel_size - 1) * cv.dilation
    if cv.stride != 1 or reach % 2 or cv.padding != reach // 2 or cv.padding_right != reach // 2:
        raise ValueError(f"{cv}: only a stride-1 Conv1d with symmetric padding (k - 1) * d / 2 streams with a look-ahead")
    return delay_in + cv.padding


def mirrored_delay(cv, delay_in):
    """:func:`lookahead_delay` for a REFLECT-padded ``Conv1d`` (the non-causal MelGAN's; the mirrored form of the
    streaming kernel): its causal form on an axis shifted by its padding, the window mirroring on read.
    ValueError for a layer that has no such form."""
    reach = (cv.kernel_size - 1) * cv.dilation
    if cv.groups != 1 or cv.pad_mode != "reflect" or cv.transposed:
        raise ValueError(f"{cv}: only a reflect-padded, ungrouped Conv1d streams through the mirrored form")
    if reach % 2:
        raise ValueError(f"{cv}: an even kernel has no symmetric padding, so it does not stream with a look-ahead")
    if cv.stride != 1 or cv.padding != reach // 2 or cv.padding_right != reach // 2:
        raise ValueError(f"{cv}: only a stride-1 Conv1d with symmetric padding (k - 1) * d / 2 streams with a look-ahead")
    return delay_in + cv.padding


def mirrored_desc(cv, batch, n, **fused):
    """Descriptor of one push of ``n`` columns through the mirrored form of the reflect-padded ``cv``: its causal
    descriptor, ``pad_mode="reflect"``."""
    return ops.make_conv_desc(batch, cv.in_channels, cv.out_channels, n, n, cv.kernel_size, 1, cv.dilation,
                              lookahead_history_columns(cv), cv.groups, transposed=False, pad_mode="reflect", **fused)


def launch_is_mirrored(launch):
    """Does this launch of a delay plan go through the mirrored entry point (a reflect-padded convolution)?"""
    return launch.conv.pad_mode == "reflect"


def launch_desc(launch, batch, n, **fused):
    """The descriptor of a plan's launch for a push of ``n`` input columns, mirrored or delayed."""
    return (mirrored_desc if launch_is_mirrored(launch) else lookahead_desc)(launch.conv, batch, n, **fused)


def lookahead_settle_frames(plan):
    """Frames that must have gone before a push for none of its launches to have an edge of the utterance in its window
    or history -- the condition under which a captured graph, whose window arguments are fixed, may be replayed:
    ``frames_before * rate >= delay + pad`` for every launch, ``pad`` being the mirror reach of a reflect-padded launch
    (its window goes ``2 * pad`` input columns back, and its input is ``pad`` columns younger than its output) and 0 for
    a zero-padded one (whose only edge is its valid window's)."""
    return max(-(-(launch.delay + (launch.conv.padding if launch_is_mirrored(launch) else 0)) // launch.rate)
               for launch in plan)


def mirrored_min_frames(plan):
    """The shortest utterance reflection can pad: every reflect-padded launch needs more input columns than its padding,
    ``frames * rate > pad`` (4 frames for a first layer of kernel 7).  1 for a plan without such a launch."""
    return max([launch.conv.padding // launch.rate + 1 for launch in plan if launch_is_mirrored(launch)] + [1])


def mirrored_in_window(launch, frames_before=None, total_frames=None):
    """Valid window ``(lo, hi)`` of a mirrored launch's INPUT, chunk-relative and unclamped: the producing launch's
    valid window, i.e. the launch's own shifted back by its padding.  ``lo < 0``: the utterance began in the history;
    ``hi`` None: its length is not known yet.  ``frames_before`` None: steady state, no edge in reach."""
    if frames_before is None:
        return -(2 ** 30), None
    start = launch.delay - launch.conv.padding - frames_before * launch.rate
    return start, (None if total_frames is None else start + total_frames * launch.rate)


def lookahead_history_columns(cv):
    """Columns of raw input the causal form of the non-causal ``cv`` keeps: ``(k - 1) * d``, 1 for a transposed layer."""
    return 1 if cv.transposed else (cv.kernel_size - 1) * cv.dilation


def lookahead_desc(cv, batch, n, **fused):
    """Descriptor of one push of ``n`` columns through the causal form of the non-causal ``cv``."""
    if cv.transposed:
        return ops.make_conv_desc(batch, cv.in_channels, cv.out_channels, n, n * cv.stride, cv.kernel_size, cv.stride, 1,
                                  cv.stride, cv.groups, transposed=True, pad_mode="zero", **fused)
    return ops.make_conv_desc(batch, cv.in_channels, cv.out_channels, n, n, cv.kernel_size, 1, cv.dilation,
                              lookahead_history_columns(cv), cv.groups, transposed=False, pad_mode="zero", **fused)


# One launch of the look-ahead walk: ``rate`` output columns per mel frame, ``delay`` of the output, ``delay1`` /
# ``delay2`` = output delay minus the delay of addend 1 / 2 (0: no addend, or one that is not delayed)
LookaheadLaunch = collections.namedtuple("LookaheadLaunch", "conv rate delay delay1 delay2")


def lookahead_state_shapes(plan, batch):
    """Shapes of the state tensors of one ping-pong half, in the order :class:`LookaheadWalk` takes them: per launch
    its history (if any), then the delay line of addend 1, then of addend 2 (where delayed)."""
    shapes = []
    for launch in plan:
        cv = launch.conv
        if lookahead_history_columns(cv):
            shapes.append((batch, cv.in_channels, lookahead_history_columns(cv)))
        shapes += [(batch, cv.out_channels, d) for d in (launch.delay1, launch.delay2) if d]
    return shapes


def lookahead_window(delay, rate, t_out, frames_before=None, total_frames=None):
    """Valid window ``(lo, hi)`` of a launch's ``t_out`` output columns (chunk-relative): the columns that hold the
    utterance on the launch's shifted axis.  ``delay`` / ``rate``: the launch's output delay and columns per mel frame;
    ``frames_before``: frames the stream took before this push (None: steady state, the window is full);
    ``total_frames``: the utterance's length once it is known (the flush), else None."""
    lo, hi = 0, t_out
    if frames_before is not None:
        before = frames_before * rate  # output columns the stream produced before this push
        lo = min(max(delay - before, 0), t_out)
        if total_frames is not None:
            hi = min(max(delay + total_frames * rate - before, 0), t_out)
    return lo, hi


class _Walk:
    """What the two walks of a delay plan share: one push through the plan's launches, each taking its state pairs in
    plan order and its valid window.  ``state_in`` (None: start of stream, every state reads as zeros) / ``state_out``:
    one ping-pong half each; ``frames_before``: frames the stream took before this push (None: steady state, every
    window is full); ``total_frames``: the utterance's length once it is known (the flush), else None; ``precision``:
    of every launch of the push -- the state tensors are the same raw fp32 in either."""

    def __init__(self, plan, state_in, state_out, frames_before=None, total_frames=None, precision="fp32"):
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"{type(self).__name__}: precision must be 'fp32' or 'bf16', got {precision!r}")
        self.precision = precision
        self._plan = iter(plan)
        self._in = None if state_in is None else iter(state_in)
        self._out = iter(state_out)
        self.frames_before, self.total_frames = frames_before, total_frames

    @property
    def at_start(self):
        """No state yet: the first push of an utterance."""
        return self._in is None

    def _pair(self):
        """The next ``(state_in, state_out)`` pair; ``state_in`` None at the start of a stream."""
        return (None if self._in is None else next(self._in), next(self._out))

    def _window(self, launch, t_out):
        return lookahead_window(launch.delay, launch.rate, t_out, self.frames_before, self.total_frames)

    def _take_conv(self, cv):
        """The next launch of a convolution plan, which must be ``cv``'s -> ``(launch, history pair, delay line pair of
        addend 1, of addend 2)``, ``(None, None)`` where the launch keeps none."""
        launch = next(self._plan)
        if launch.conv is not cv:
            raise RuntimeError(f"look-ahead walk out of step: the plan expects {launch.conv}, the model ran {cv}")
        hist = self._pair() if lookahead_history_columns(cv) else (None, None)
        line1, line2 = (self._pair() if d else (None, None) for d in (launch.delay1, launch.delay2))
        return launch, hist, line1, line2


class LookaheadWalk(_Walk):
    """The walk of a convolution plan (HiFi-GAN, MelGAN): hands every launch its state tensors, of
    :func:`lookahead_state_shapes`, and its valid window, and runs it.  ``precision="bf16"``: every launch runs with
    bf16 operands on the layer's bf16 image (csrc/conv1d_stream_bf16.hip, the delayed form)."""

    def run(self, cv, x, add1=None, add2=None, **fused):
        """The next launch of the plan, which must be ``cv``'s, on the chunk ``x``; fused-epilogue keywords as in
        ``forward``.  A reflect-padded launch (the non-causal MelGAN's) goes through the mirrored form, whose input
        window is the producing launch's unclamped valid window: fp32 only, no addends."""
        launch, hist, line1, line2 = self._take_conv(cv)
        desc = launch_desc(launch, x.shape[0], x.shape[-1], **fused)
        valid = self._window(launch, desc.t_out)
        if not launch_is_mirrored(launch):
            return _launch("delayed", self.precision, cv, desc, x, hist, add1, line1, launch.delay1, add2, line2,
                           launch.delay2, valid, delays=(launch.delay1, launch.delay2))
        if add1 is not None or add2 is not None or launch.delay1 or launch.delay2:
            raise RuntimeError("the mirrored form of the streaming kernel takes no addends")
        return _launch("mirrored", self.precision, cv, desc, x, hist,
                       mirrored_in_window(launch, self.frames_before, self.total_frames), valid)


class SlotWalk(_Walk):
    """:class:`LookaheadWalk` for a batch whose items sit at different points of different utterances
    (utils.StreamPool): ``run`` has the same contract, but every launch goes through the slotted form
    and derives each item's valid window itself, from ``slots`` -- the device table of ``ops.conv1d_stream_slots_forward``,
    one row per item -- and its own rate and delay.  There is no start-of-stream walk: ``state_in`` is always a half, and
    an item that starts an utterance is fresh in the table.  A reflect-padded launch (utils.MelGANStreamPool, DESIGN.md
    s11.12) goes through the slotted-mirrored form, which also derives each item's input edges from the table: fp32
    only, no addends."""

    def __init__(self, plan, state_in, state_out, slots, precision="fp32"):
        if state_in is None:
            raise ValueError("SlotWalk: state_in is a ping-pong half; the start of a stream is an item's, in the table")
        super().__init__(plan, state_in, state_out, precision=precision)
        self.slots = slots

    def run(self, cv, x, add1=None, add2=None, **fused):
        launch, hist, line1, line2 = self._take_conv(cv)
        if launch_is_mirrored(launch):
            if add1 is not None or add2 is not None or launch.delay1 or launch.delay2:
                raise RuntimeError("the mirrored form of the streaming kernel takes no addends")
            desc = mirrored_desc(cv, x.shape[0], x.shape[-1], **fused)
            return _launch("slots_mirrored", self.precision, cv, desc, x, hist, self.slots, launch.rate, launch.delay)
        desc = lookahead_desc(cv, x.shape[0], x.shape[-1], **fused)
        return _launch("slots", self.precision, cv, desc, x, hist, add1, line1, launch.delay1, add2, line2, launch.delay2,
                       self.slots, launch.rate, launch.delay, delays=(launch.delay1, launch.delay2))


# ---- the same for the NON-causal Parallel WaveGAN generator (utils.PWGLookaheadStream).  Its launches
# are not all convolutions (upsampler stages, gated layers, delay lines), so a launch names its kind and module and lists
# its state itself: ``state`` = the ``(channels, columns)`` of every state tensor it keeps, in the order it takes them;
# ``c_delay``: how late a gated layer reads the conditioning (0 for every other launch).
PWGLookaheadLaunch = collections.namedtuple("PWGLookaheadLaunch", "kind module rate delay c_delay state")


def pwg_lookahead_state_shapes(plan, batch):
    """Shapes of the state tensors of one ping-pong half, in the order :class:`PWGLookaheadWalk` takes them."""
    return [(batch, ch, cols) for launch in plan for ch, cols in launch.state]


# Where the items of a launch stand, as a slotted walk hands it out in the place of the valid window ``(lo, hi)``: the
# device table (one row per item), the launch's rate and output delay -- the kernel derives every item's window itself
# (utils.PWGStreamPool).  ``seed``: for ``conv_in`` with a context window the table whose fresh running
# items get their first frame replicated into the history in front of the launch (``slots`` is then the second table,
# in which no item is fresh); None for every other launch.
SlotPosition = collections.namedtuple("SlotPosition", "slots rate delay seed")

# ---- the rule of a Parallel WaveGAN stream launch that is no convolution, by the rule of ``_STREAM_KERNELS``: a kind's
# row per form; the position decides the form and how it is passed -- ``valid=(lo, hi)`` or the table, rate and delay
_PWG_STREAM_KERNELS = {
    ("stage", "delayed"): ops.stretch_conv_stream_delayed,
    ("stage", "slots"): ops.stretch_conv_stream_slots,
    ("layer", "delayed", "fp32"): ops.wavenet_stream_delayed_forward,
    ("layer", "delayed", "bf16"): ops.wavenet_stream_delayed_forward_bf16,
    ("layer", "slots", "fp32"): ops.wavenet_stream_slots_forward,
    ("layer", "slots", "bf16"): ops.wavenet_stream_slots_forward_bf16,
}


def _position(valid):
    """``(form, keywords)`` of the position a walk handed out."""
    if isinstance(valid, SlotPosition):
        return "slots", {"slots": valid.slots, "rate": valid.rate, "delay": valid.delay}
    return "delayed", {"valid": valid}


def pwg_stream_launch(kind, valid, *args, precision=None):
    """One launch of ``kind`` ("stage": an upsampler stage, fp32 in either precision; "layer": a gated layer, in
    ``precision``) of the Parallel WaveGAN look-ahead walk on ``args``, what its entry takes in front of the position;
    ``valid``: what the walk handed out, a window (lock-step) or a :class:`SlotPosition` (a pool)."""
    form, where = _position(valid)
    return _PWG_STREAM_KERNELS[(kind, form) if precision is None else (kind, form, precision)](*args, **where)


def lookahead_line(x, pair, position=None, delayed=False):
    """A delay line of the Parallel WaveGAN look-ahead walk on the chunk ``x``: ``pair = (line_in, line_out)``;
    ``position``: what the walk handed out -- a line has no window, a slotted one reads fresh and paused from the table."""
    if isinstance(position, SlotPosition):
        return ops.delay_line_slots_forward(x, pair[0], pair[1], position.slots, delayed=delayed)
    return ops.delay_line_forward(x, pair[0], pair[1], delayed=delayed)


def lookahead_launch(cv, desc, x, hist=(None, None), valid=None, precision="fp32"):
    """One delayed launch of ``cv`` under ``desc`` without addends: the history pair and the valid window are the
    caller's (``conv_in`` and the 1 x 1 convolutions of the Parallel WaveGAN look-ahead stream); a :class:`SlotPosition`
    in the window's place: the slotted form.  ``precision``, a module in bf16 mode and a layer the kernel does not
    cover: by the rule of :func:`_launch`."""
    form, where = _position(valid)
    return _launch(form, precision, cv, desc, x, hist, **where)


def pointwise_desc(cv, batch, n, **fused):
    """Descriptor of an unpadded 1 x 1 ``Conv1d`` on ``n`` columns of a stream (no history)."""
    return ops.make_conv_desc(batch, cv.in_channels, cv.out_channels, n, n, 1, cv.stride, 1, 0, cv.groups,
                              transposed=False, pad_mode="zero", **fused)


def lookahead_pointwise(cv, x, valid, precision="fp32", **fused):
    """A 1 x 1 ``Conv1d`` on the next columns of a look-ahead stream: :func:`stream_pointwise` with a valid window, which
    keeps the bias out of the padding."""
    if cv.kernel_size != 1 or cv.padding != 0 or cv.padding_right != 0:
        raise ValueError("lookahead_pointwise: not an unpadded 1 x 1 convolution")
    return lookahead_launch(cv, pointwise_desc(cv, x.shape[0], x.shape[-1], **fused), x, valid=valid, precision=precision)


class PWGLookaheadWalk(_Walk):
    """The walk of ``ParallelWaveGANGenerator.lookahead_plan()``: hands every launch its state pairs, of
    :func:`pwg_lookahead_state_shapes`, and its valid window; the model runs it.  ``precision="bf16"``: the model runs
    every convolution and gated layer of the push with bf16 operands."""

    def take(self, kind, module, frames):
        """The next launch of the plan, which must be ``(kind, module)``, on a chunk of ``frames`` mel frames ->
        ``(launch, [(state_in, state_out), ...], (lo, hi))``: its state pairs (``state_in`` None at the start of a stream)
        and the valid window of its ``frames * launch.rate`` output columns."""
        launch = next(self._plan)
        if launch.kind != kind or launch.module is not module:
            raise RuntimeError(f"look-ahead walk out of step: the plan expects {launch.kind} {launch.module}, the model "
                               f"ran {kind} {module}")
        return launch, [self._pair() for _ in launch.state], self._window(launch, frames * launch.rate)


def slot_table_rows_in(rows):
    """The second table of a Parallel WaveGAN pool's step, from the rows of the first: ``(before + 1, left - 1, flags,
    own)``.  ``conv_in``, launched with ``delay + rate`` over it, gets the windows of ``delay`` over the first --
    ``delay + rate - (before + 1) * rate = delay - before * rate``, ``delay + rate + (left - 1) * rate = delay + left *
    rate`` -- and no item of it is fresh, so the history the seeding kernel wrote is read."""
    return [(before + 1, left - 1, flags, own) for before, left, flags, own in rows]


class PWGSlotWalk(_Walk):
    """:class:`PWGLookaheadWalk` for a batch whose items sit at different points of different utterances
    (utils.PWGStreamPool): ``take`` has the same contract, but hands out a :class:`SlotPosition` --
    the device table ``slots``, the launch's rate and delay -- where the lock-step walk hands out the valid window, and
    the model launches the slotted form.  ``slots_in``: the second table (:func:`slot_table_rows_in`), which ``conv_in``
    with a context window takes with ``delay + rate`` behind the seeding kernel; None for a plan whose ``conv_in`` keeps
    no history.  There is no start-of-stream walk: ``state_in`` is always a half, and an item that starts an utterance
    is fresh in the table."""

    def __init__(self, plan, state_in, state_out, slots, slots_in=None, precision="fp32"):
        if state_in is None:
            raise ValueError("PWGSlotWalk: state_in is a ping-pong half; the start of a stream is an item's, in the table")
        super().__init__(plan, state_in, state_out, precision=precision)
        self.slots, self.slots_in = slots, slots_in

    def take(self, kind, module, frames):
        """The next launch of the plan, which must be ``(kind, module)`` -> ``(launch, [(state_in, state_out), ...],
        SlotPosition)``; ``frames`` is the lock-step walk's and not needed here: the kernel knows its columns."""
        launch = next(self._plan)
        if launch.kind != kind or launch.module is not module:
            raise RuntimeError(f"look-ahead walk out of step: the plan expects {launch.kind} {launch.module}, the model "
                               f"ran {kind} {module}")
        pairs = [self._pair() for _ in launch.state]
        if kind == "conv_in" and pairs:
            if self.slots_in is None:
                raise RuntimeError("PWGSlotWalk: conv_in keeps a history and needs the second table (slots_in)")
            return launch, pairs, SlotPosition(self.slots_in, launch.rate, launch.delay + launch.rate, self.slots)
        return launch, pairs, SlotPosition(self.slots, launch.rate, launch.delay, None)
